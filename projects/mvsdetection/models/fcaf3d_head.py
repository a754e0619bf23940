"""FCAF3D neck + head on the HIP sparse engine.

Registered name, constructor signature, forward outputs, pruning rule, box decoding and the raw-box dump follow
the reference's projects/mvsdetection/models/fcaf3d_head.py (FCAF3DHead :24-349, compute_centerness :395-402,
FCAF3DAssigner :405-484).  Parameter names match (up_block_i.0.kernel, out_block_i.1.bn.*, centerness_conv.kernel,
reg_conv.kernel, cls_conv.kernel/bias, scales.i.scale).  Training losses (:142-214) need mmdet's loss registry and
are a "next" row of SURVEY.md 8(f); the assigner is provided because it is pure tensor math."""
import os

import numpy as np
import torch
from torch import nn

from cnrma_amd import nn as snn
from cnrma_amd import plan as P
from cnrma_amd import sparse as S

from ..registry import BBOX_ASSIGNERS, HEADS, HAVE_MMDET, build_assigner


class Scale(nn.Module):
    """mmcv.cnn.Scale: a learnable scalar factor (key: `scale`)."""

    def __init__(self, scale=1.0):
        super().__init__()
        self.scale = nn.Parameter(torch.tensor(scale, dtype=torch.float))

    def forward(self, x):
        return x * self.scale


class _TestCfg(dict):
    """test_cfg with attribute access (mmcv.Config style): missing keys read as None; dunder look-ups fall through, so that
    copy.deepcopy / pickle of the head work"""

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return self.get(name)


def _without_type(cfg):
    return {k: v for k, v in dict(cfg).items() if k not in ("type", "use_sigmoid")}


class _SigmoidFocalLoss(nn.Module):
    """mmdet FocalLoss(use_sigmoid=True): sum over rows and classes of alpha_t (1 - p_t)^gamma BCE / avg_factor;
    label < 0 (or >= n_classes) = background row (all-zero target)."""

    def __init__(self, gamma=2.0, alpha=0.25, loss_weight=1.0, **_):
        super().__init__()
        self.gamma, self.alpha, self.loss_weight = gamma, alpha, loss_weight

    def forward(self, pred, labels, avg_factor=None):
        t = torch.zeros_like(pred)
        pos = (labels >= 0) & (labels < pred.shape[1])
        t[pos.nonzero().view(-1), labels[pos].long()] = 1.0
        p = pred.sigmoid()
        pt = (1 - p) * t + p * (1 - t)
        w = (self.alpha * t + (1 - self.alpha) * (1 - t)) * pt.pow(self.gamma)
        loss = nn.functional.binary_cross_entropy_with_logits(pred, t, reduction="none") * w
        return self.loss_weight * loss.sum() / (avg_factor if avg_factor is not None else max(loss.numel(), 1))


class _SigmoidBCELoss(nn.Module):
    """mmdet CrossEntropyLoss(use_sigmoid=True): BCE with logits, summed / avg_factor"""

    def __init__(self, loss_weight=1.0, **_):
        super().__init__()
        self.loss_weight = loss_weight

    def forward(self, pred, target, avg_factor=None):
        # at least float32, and float64 under float64 logits: torch evaluates (1 - target) * pred in place in the target's type, so
        # a float32 target would round a float64 evaluation of this loss to float32
        target = target.to(torch.promote_types(pred.dtype, torch.float32))
        loss = nn.functional.binary_cross_entropy_with_logits(pred, target, reduction="none")
        return self.loss_weight * loss.sum() / (avg_factor if avg_factor is not None else max(loss.numel(), 1))


class _IoU3DLoss(nn.Module):
    """IoU3DLoss of the FCAF3D code base: (1 - IoU3D) of (cx, cy, cz, dx, dy, dz[, yaw]) boxes, weighted, / avg_factor.
    with_yaw=False: axis-aligned boxes (ScanNet); with_yaw=True: rotated about z (ARKit) through core/rotated_iou.py."""

    def __init__(self, loss_weight=1.0, with_yaw=False, **_):
        super().__init__()
        self.loss_weight, self.with_yaw = loss_weight, with_yaw

    def forward(self, pred, target, weight=None, avg_factor=None):
        if self.with_yaw and pred.shape[1] >= 7:
            from ..core.rotated_iou import rotated_iou_3d
            iou = rotated_iou_3d(pred[:, :7], target[:, :7].to(pred.dtype))
        else:
            target = target.to(pred.dtype)                      # like the rotated branch: a float64 evaluation upcasts the targets first
            p_lo, p_hi = pred[:, :3] - pred[:, 3:6] / 2, pred[:, :3] + pred[:, 3:6] / 2
            t_lo, t_hi = target[:, :3] - target[:, 3:6] / 2, target[:, :3] + target[:, 3:6] / 2
            # products written out: prod()'s backward reads a scalar back (a host synchronisation inside loss.backward())
            ov = (torch.min(p_hi, t_hi) - torch.max(p_lo, t_lo)).clamp(min=0)
            inter = ov[:, 0] * ov[:, 1] * ov[:, 2]
            union = pred[:, 3] * pred[:, 4] * pred[:, 5] + target[:, 3] * target[:, 4] * target[:, 5] - inter
            iou = inter / union.clamp(min=1e-8)
        loss = 1 - iou
        if weight is not None:
            loss = loss * weight
        return self.loss_weight * loss.sum() / (avg_factor if avg_factor is not None else max(loss.numel(), 1))


from ..core.boxes import GTBoxes  # noqa: E402,F401  (kept importable from here: tests and the detector use it)


def _cut_ids(cls, cen, nms_pre, n_dev=None):
    """the pre-NMS cut of one scene's rows on one level (reference :247-256): more than nms_pre > 0 rows give the ids of the
    nms_pre best by max class score x centerness (the ranking key only), best first, equal scores by ascending row index
    (torch.topk leaves ties open); anything else gives None: every row, in row order.  n_dev (static trace): len(cls) is a
    capacity and the rows behind the live count rank -inf; fewer than nms_pre live rows all come, best first, in front of
    slots that repeat row 0."""
    return S.topk_indices(S.max_scores(cls, cen), nms_pre, n_dev) if len(cls) > nms_pre > 0 else None


def _rank_by_scene(scene, max_scores):
    """the cut for several scenes in one row set: the rows by ONE stable sort on the key (scene, descending score).  The scores
    are >= 0, so their bit patterns order them; equal scores stay in row order.  Every scene's rows become one contiguous run,
    best first; rows given the scene id n_scenes (the dead rows of a static trace) sort behind every scene.  The first nms_pre
    rows of a run are what _cut_ids gives for that scene alone; the run of a scene that is not cut goes back into row order (a
    sort of its ids).  That is the caller's part: it finds the runs with host counts or through device-side offsets."""
    return torch.sort((scene.long() << 32) | (0xFFFFFFFF - max_scores.view(torch.int32).long()), stable=True)[1]


@HEADS.register_module()
class FCAF3DHead(nn.Module):
    def __init__(self, n_classes, in_channels, out_channels, n_reg_outs, voxel_size, pts_threshold, assigner,
                 yaw_parametrization="fcaf3d",
                 loss_centerness=dict(type="CrossEntropyLoss", use_sigmoid=True, loss_weight=1.0),
                 loss_bbox=dict(type="IoU3DLoss", loss_weight=1.0),
                 loss_cls=dict(type="FocalLoss", use_sigmoid=True, gamma=2.0, alpha=0.25, loss_weight=1.0),
                 train_cfg=None, test_cfg=None, device_targets=False):
        super().__init__()
        self.fp16_enabled = False
        self.device_targets = bool(device_targets)      # True: targets and losses by the HIP kernels, no host read under loss()
        self.voxel_size = voxel_size
        self.yaw_parametrization = yaw_parametrization
        self.assigner = build_assigner(assigner) if assigner is not None else None
        if HAVE_MMDET:
            from mmdet.models.builder import build_loss
            self.loss_centerness, self.loss_bbox, self.loss_cls = map(build_loss, (loss_centerness, loss_bbox, loss_cls))
        else:   # the three losses the configs name, restated in torch (mmdet / mmdet3d are third-party: unpinned)
            self.loss_centerness = _SigmoidBCELoss(**_without_type(loss_centerness))
            self.loss_bbox = _IoU3DLoss(**_without_type(loss_bbox))
            self.loss_cls = _SigmoidFocalLoss(**_without_type(loss_cls))
        self.train_cfg = train_cfg
        self.test_cfg = _TestCfg(test_cfg) if isinstance(test_cfg, dict) else test_cfg
        self.pts_threshold = pts_threshold
        self.n_classes, self.n_reg_outs = n_classes, n_reg_outs
        self._init_layers(in_channels, out_channels, n_reg_outs, n_classes)
        self._fused_head = None

    # ---- layers (reference :61-98) -------------------------------------------------------------------------
    @staticmethod
    def _make_block(cin, cout):
        return snn.FusedSequential(snn.MinkowskiConvolution(cin, cout, kernel_size=3, dimension=3),
                                   snn.MinkowskiBatchNorm(cout), snn.MinkowskiELU())

    @staticmethod
    def _make_up_block(cin, cout):
        return snn.FusedSequential(
            snn.MinkowskiGenerativeConvolutionTranspose(cin, cout, kernel_size=2, stride=2, dimension=3),
            snn.MinkowskiBatchNorm(cout), snn.MinkowskiELU(),
            snn.MinkowskiConvolution(cout, cout, kernel_size=3, dimension=3),
            snn.MinkowskiBatchNorm(cout), snn.MinkowskiELU())

    def _init_layers(self, in_channels, out_channels, n_reg_outs, n_classes):
        self.pruning = snn.MinkowskiPruning()
        for i in range(len(in_channels)):
            if i > 0:
                setattr(self, f"up_block_{i}", self._make_up_block(in_channels[i], in_channels[i - 1]))
            setattr(self, f"out_block_{i}", self._make_block(in_channels[i], out_channels))
        self.centerness_conv = snn.MinkowskiConvolution(out_channels, 1, kernel_size=1, dimension=3)
        self.reg_conv = snn.MinkowskiConvolution(out_channels, n_reg_outs, kernel_size=1, dimension=3)
        self.cls_conv = snn.MinkowskiConvolution(out_channels, n_classes, kernel_size=1, bias=True, dimension=3)
        self.scales = nn.ModuleList([Scale(1.0) for _ in range(len(in_channels))])

    def init_weights(self):
        nn.init.normal_(self.centerness_conv.kernel, std=.01)
        nn.init.normal_(self.reg_conv.kernel, std=.01)
        nn.init.normal_(self.cls_conv.kernel, std=.01)
        nn.init.constant_(self.cls_conv.bias, float(-np.log((1 - 0.01) / 0.01)))   # bias_init_with_prob(.01)
        self._fused_head = None

    def train(self, mode=True):
        self._fused_head = None
        return super().train(mode)

    # ---- forward (reference :107-139, :275-298) ---------------------------------------------------------------
    def forward(self, x, fused=False):
        """fused=True (eval only): several scenes stay in ONE row set per level -- every output list has a single entry
        and a fifth list holds the level's coordinate set (scene ids, cached rows per scene); decode with
        get_bboxes_fused()."""
        outs = []
        inputs = x
        x = inputs[-1]
        scores = None
        for i in range(len(inputs) - 1, -1, -1):
            if i < len(inputs) - 1:
                x = getattr(self, f"up_block_{i + 1}")(x)
                x = inputs[i] + x                       # coordinate union, features added (:114)
                x = self._prune(x, scores)
            out = getattr(self, f"out_block_{i}")(x)
            out = self.forward_single(out, self.scales[i], fused)
            scores = out[-1]
            outs.append(out[:-1] + ([out[-1].cs],) if fused else out[:-1])
        return zip(*outs[::-1])

    def _prune(self, x, scores):
        """keep the top `pts_threshold` rows per scene by the interpolated max-class score of the coarser level (reference
        :123-139; the rule and its one body: _keep_mask).  pts_threshold < 0 switches the step off; a step that keeps every row
        returns x itself.  Eagerly the host counts decide that, and the decision is recorded in the plan.  Static trace: the plan
        flag True (no calibration scene was pruned) skips and registers `rows per scene <= pts_threshold`; False and None prune
        under the live-count word, into a capacity of min(B * pts_threshold, capacity of x).  tests/test_head_select_gpu.py."""
        T, B, plan = self.pts_threshold, x.cs.n_batch, P.current()
        if T < 0:
            return x
        static = plan is not None and plan.static
        counts = None if static else x.cs.batch_counts()
        if static:                                   # the branch of the calibration run, its premise registered as an assumption
            skip = plan.next_flag()                  # True: no calibration scene needed pruning; None (scenes differ) -> prune
            if skip and B <= 1:
                plan.watch(x.cs.n_dev, 0, T)
            elif skip:                               # several scenes per pass: the premise holds per scene
                cnt, _ = x.cs.counts_dev()
                for b in range(B):
                    plan.watch(cnt[b:b + 1], 0, T)
        else:
            skip = all(c <= T for c in counts)
            if plan is not None:
                plan.record_flag(skip)
        if skip:
            return x                                 # the top-k keeps every row: pruning is the identity
        mask = self._keep_mask(x, scores, counts)
        if static:
            return S.prune(x, mask, n_keep=min(B * T, x.cs.n))
        kept = [min(c, T) for c in counts]           # the mask holds exactly min(n, threshold) rows per scene
        return S.prune(x, mask, n_keep=sum(kept), counts=kept)

    @torch.no_grad()
    def _keep_mask(self, x, scores, counts=None):
        """uint8 keep-mask of the pruning step: per scene the min(n, pts_threshold) rows of x with the largest interpolated score;
        of rows with equal scores those with the smaller row index stay (the reference's topk(sorted=False) leaves the choice
        open).  A radix select (S.topk_mask) instead of torch.topk's sort, under the live-count word x.cs.n_dev (None in the
        eager forms; rows behind it are never kept).  Several scenes: one select per scene with the other scenes' rows ranked
        -inf.  counts (host rows per scene, eager forms): a scene at or below the threshold keeps its rows without a select."""
        T, n_dev = self.pts_threshold, x.cs.n_dev
        interpolated = S.interpolate(scores, x.C, n_dev)
        if x.cs.n_batch <= 1:
            return S.topk_mask(interpolated, T, n_dev=n_dev)         # keeps every row when n <= threshold
        flat, scene = interpolated.view(-1), x.C[:, 0]
        low = torch.full_like(flat, float("-inf"))
        mask = None
        for b in range(x.cs.n_batch):
            mine = scene == b
            if counts is not None and counts[b] <= T:
                m = mine.to(torch.uint8)
            else:
                m = S.topk_mask(torch.where(mine, flat, low), T, n_dev=n_dev)
                if counts is None:                   # the scene may hold fewer rows than the threshold: the select then also
                    m = m & mine.to(torch.uint8)     # keeps rows ranked -inf, which are the other scenes'
            mask = m if mask is None else mask | m
        return mask

    def _head_weights(self):
        """the three 1x1 head convolutions as ONE [128, 1+R+n_cls] GEMM (+ bias row for the class logits)"""
        params = (self.centerness_conv.kernel, self.reg_conv.kernel, self.cls_conv.kernel, self.cls_conv.bias)
        tag = tuple((t.data_ptr(), t._version, t.device) for t in params)       # in-place updates / load_state_dict bump _version
        if self._fused_head is None or self._fused_head[2] != tag:
            with torch.no_grad():
                w = torch.cat((self.centerness_conv.kernel, self.reg_conv.kernel, self.cls_conv.kernel), dim=1)
                n_out = w.shape[1]
                pad = (-n_out) % 4                       # 16-byte rows: the conv kernel's branch-free staging path
                w = torch.cat((w, w.new_zeros(w.shape[0], pad)), dim=1).contiguous()
                b = torch.zeros(w.shape[1], device=w.device)
                b[1 + self.n_reg_outs:n_out] = self.cls_conv.bias.view(-1)
            self._fused_head = (w, b.contiguous(), tag)
        return self._fused_head[:2]

    def forward_single(self, x, scale, fused=False):
        if self.training or (x.cs.n_batch > 1 and not fused):
            if self.training:
                centerness = self.centerness_conv(x).F
                cls_score = self.cls_conv(x).F
                reg_final = self.reg_conv(x).F
            else:
                w, b = self._head_weights()
                y = S.conv(x, w, kernel_size=1, shift=b).F
                n_out = 1 + self.n_reg_outs + self.n_classes
                centerness, reg_final, cls_score = y[:, :1], y[:, 1:1 + self.n_reg_outs], y[:, 1 + self.n_reg_outs:n_out]
            prune_scores = S.SparseTensor(S.row_max(cls_score.contiguous()), x.cs)           # :279-282
            reg_distance = torch.exp(scale(reg_final[:, :6]))                                  # :284
            bbox_pred = torch.cat((reg_distance, reg_final[:, 6:]), dim=1)                     # :285-286
            perms = x.decomposition_permutations
            # index_select: its backward is an index_add (advanced indexing's sorts, far slower on large row sets)
            centernesses = [centerness.index_select(0, p) for p in perms]
            bbox_preds = [bbox_pred.index_select(0, p) for p in perms]
            cls_scores = [cls_score.index_select(0, p) for p in perms]
            points = [c * self.voxel_size for c in x.decomposed_coordinates]                   # :294-296
            return centernesses, bbox_preds, cls_scores, points, prune_scores
        # single scene, eval: the three 1x1 convolutions are ONE GEMM and the whole tail is one kernel
        w, b = self._head_weights()
        y = S.conv(x, w, kernel_size=1, shift=b).F
        cen, box, cls, mx, pts = S.head_post(y, x.C, self.n_reg_outs, self.n_classes, scale.scale, self.voxel_size)
        return [cen], [box], [cls], [pts], S.SparseTensor(mx, x.cs)

    # ---- decoding (reference :217-271, :300-349) -----------------------------------------------------------------
    def _bbox_pred_to_bbox(self, points, bbox_pred):
        if bbox_pred.shape[0] == 0:
            return bbox_pred
        if torch.is_grad_enabled() and bbox_pred.requires_grad:       # training: the same formulas in torch (:300-349)
            b, p = bbox_pred, points
            ctr = torch.stack((p[:, 0] + (b[:, 1] - b[:, 0]) / 2, p[:, 1] + (b[:, 3] - b[:, 2]) / 2,
                               p[:, 2] + (b[:, 5] - b[:, 4]) / 2), dim=-1)
            if b.shape[1] == 6:
                return torch.cat((ctr, torch.stack((b[:, 0] + b[:, 1], b[:, 2] + b[:, 3], b[:, 4] + b[:, 5]), -1)), dim=-1)
            if self.yaw_parametrization == "naive":
                return torch.cat((ctr, torch.stack((b[:, 0] + b[:, 1], b[:, 2] + b[:, 3], b[:, 4] + b[:, 5]), -1), b[:, 6:7]), -1)
            if self.yaw_parametrization == "sin-cos":
                norm = torch.sqrt(b[:, 6:7] ** 2 + b[:, 7:8] ** 2)
                size = torch.stack((b[:, 0] + b[:, 1], b[:, 2] + b[:, 3], b[:, 4] + b[:, 5]), -1)
                return torch.cat((ctr, size, torch.atan2(b[:, 6:7] / norm, b[:, 7:8] / norm)), -1)
            scale = b[:, 0] + b[:, 1] + b[:, 2] + b[:, 3]
            q = torch.exp(torch.sqrt(b[:, 6] ** 2 + b[:, 7] ** 2))
            return torch.cat((ctr, torch.stack((scale / (1 + q), scale / (1 + q) * q, b[:, 5] + b[:, 4],
                                                0.5 * torch.atan2(b[:, 6], b[:, 7])), -1)), dim=-1)
        return S.decode_boxes(points.float(), bbox_pred, self.yaw_parametrization)

    @property
    def nms_pre(self):
        """rows per scene and level that the pre-NMS cut lets through (0, also for a missing test config or key: no cut)"""
        return (self.test_cfg.nms_pre or 0) if self.test_cfg is not None else 0

    @staticmethod
    def _fused_levels(*lists):
        """level by level, the single entries of the output lists of forward(..., fused=True)"""
        for level in zip(*lists):
            yield [entries[0] for entries in level]

    def _decode_into(self, boxes, scores, ids, cls, cen, box, pts):
        """boxes and class scores of the rows `ids` (None: every row) of one level, appended to the two lists"""
        bx, sc = S.select_decode(ids, cls, cen, box, pts, self.yaw_parametrization)
        boxes.append(bx)
        scores.append(sc)

    def _get_bboxes_single(self, centernesses, bbox_preds, cls_scores, points, scene_id=None, save_path=None):
        """one scene's levels through the cut (_cut_ids) and the decode; under a recording plan one flag per level: was it cut?"""
        mlvl_bboxes, mlvl_scores = [], []
        plan, nms_pre = P.current(), self.nms_pre
        for centerness, bbox_pred, cls_score, point in zip(centernesses, bbox_preds, cls_scores, points):
            if plan is not None:
                plan.record_flag(len(cls_score) > nms_pre > 0)
            self._decode_into(mlvl_bboxes, mlvl_scores, _cut_ids(cls_score, centerness, nms_pre), cls_score, centerness, bbox_pred, point)
        bboxes, scores = torch.cat(mlvl_bboxes), torch.cat(mlvl_scores)
        if save_path is not None:
            save_place = os.path.join(save_path, scene_id)
            os.makedirs(save_place, exist_ok=True)
            np.savez(os.path.join(save_place, scene_id + "_bbox_raw.npz"), bboxes=bboxes.detach().cpu().numpy(),
                     scores=scores.detach().cpu().numpy())                                  # :266-271
        return bboxes, scores

    def get_bboxes(self, centernesses, bbox_preds, cls_scores, points, scene_ids, save_path):
        return [self.get_bboxes_scene(centernesses, bbox_preds, cls_scores, points, i,
                                      scene_ids[i] if scene_ids is not None else None, save_path)
                for i in range(len(centernesses[0]))]

    def get_bboxes_scene(self, centernesses, bbox_preds, cls_scores, points, i=0, scene_id=None, save_path=None):
        """_get_bboxes_single on scene i of the head's output lists (per level a list with one entry per scene)"""
        return self._get_bboxes_single(*([x[i] for x in level_lists] for level_lists in (centernesses, bbox_preds, cls_scores, points)),
                                       scene_id, save_path)

    def get_bboxes_static(self, centernesses, bbox_preds, cls_scores, points, coord_sets):
        """_get_bboxes_single inside the static trace (plan.Plan; one scene, forward(..., fused=True) outputs): no row
        count is read back.  Per level the branch of the calibration run is replayed -- cut (_cut_ids under the live-count
        word) or all rows -- and its premise registered.  Returns (bboxes [K,6|7], scores [K,n_cls], valid int32 [L], sizes):
        level l owns rows [sum(sizes[:l]), +sizes[l]) of which the first valid[l] are detections, in the order of _cut_ids.
        Flag True: sizes[l] = nms_pre, valid[l] = min(n, nms_pre), premise n > nms_pre.  Flag False (and nms_pre <= 0): sizes[l]
        = the capacity, valid[l] = n, premise n <= nms_pre.  Flag None (the calibration scenes disagreed) on a capacity above
        nms_pre: the cut form, which is valid on both sides -- the one deviation from the reference's order: n <= nms_pre live
        rows come best first instead of in row order (the same row set, valid[l] = n).  tests/test_head_select_gpu.py."""
        plan, nms_pre = P.current(), self.nms_pre
        boxes, scores, valid, sizes = [], [], [], []
        for cen, box, cls, pts, cs in self._fused_levels(centernesses, bbox_preds, cls_scores, points, coord_sets):
            cap, n_dev = cs.n, cs.n_dev
            flag = plan.next_flag()
            if flag or (flag is None and cap > nms_pre > 0):
                assert cap > nms_pre
                plan.watch(n_dev, nms_pre + 1 if flag else 0, cap)
                ids, k = _cut_ids(cls, cen, nms_pre, n_dev), nms_pre
                valid.append(torch.clamp(n_dev.view(1), max=nms_pre).to(torch.int32))
            else:
                plan.watch(n_dev, 0, min(cap, nms_pre) if nms_pre > 0 else cap)
                ids, k = None, cap
                valid.append(n_dev.view(1))
            self._decode_into(boxes, scores, ids, cls, cen, box, pts)
            sizes.append(k)
        return torch.cat(boxes), torch.cat(scores), torch.cat(valid), sizes

    def get_bboxes_static_multi(self, centernesses, bbox_preds, cls_scores, points, coord_sets, n_scenes):
        """get_bboxes_static for several scenes in one row set per level (static trace of pipeline.StaticBatch): per level ONE
        sort (_rank_by_scene, dead rows behind every scene), each scene's run found through the device-side offsets; B radix
        selects per level cost 4x as much.  The plan's flags (the single-scene branches of the calibration) are consumed and not
        needed.  Returns (bboxes [B,K,6|7], scores [B,K,n_cls], valid int32 [B,L], sizes): scene b / level l owns rows
        [sum(sizes[:l]), +sizes[l]) of block b, of which the first valid[b,l] are detections, in the order of _cut_ids."""
        plan, nms_pre, B = P.current(), self.nms_pre, n_scenes
        boxes, scores, valid, sizes = [[] for _ in range(B)], [[] for _ in range(B)], [[] for _ in range(B)], []
        for cen, box, cls, pts, cs in self._fused_levels(centernesses, bbox_preds, cls_scores, points, coord_sets):
            plan.next_flag()
            cap, n_dev = cs.n, cs.n_dev
            k = min(nms_pre, cap) if nms_pre > 0 else cap
            cnt, _ = cs.counts_dev()
            ms = S.max_scores(cls, cen)
            live = torch.arange(cap, device=ms.device, dtype=torch.int32) < n_dev
            order = _rank_by_scene(torch.where(live, cs.C[:, 0], torch.full_like(cs.C[:, 0], B)), ms)
            off = torch.cumsum(cnt, 0) - cnt
            slot = plan.const(lambda: torch.arange(k, device=ms.device, dtype=torch.int64))
            big = plan.const(lambda: torch.full((k,), cap, device=ms.device, dtype=torch.int64))
            for b in range(B):
                ids = order.index_select(0, (off[b:b + 1].long() + slot).clamp_(max=cap - 1))   # scene b's best, in score order
                nb = torch.clamp(cnt[b:b + 1], max=k)
                asc = torch.sort(torch.where(slot < nb, ids, big))[0].clamp_(max=cap - 1)         # the same rows in row order
                ids = torch.where(cnt[b:b + 1] <= k, asc, ids)
                self._decode_into(boxes[b], scores[b], ids, cls, cen, box, pts)
                valid[b].append(nb.to(torch.int32))
            sizes.append(k)
        return (torch.stack([torch.cat(x) for x in boxes]), torch.stack([torch.cat(x) for x in scores]),
                torch.stack([torch.cat(v) for v in valid]), sizes)

    def get_bboxes_fused(self, centernesses, bbox_preds, cls_scores, points, scenes, n_scenes):
        """decode of forward(..., fused=True): per level ONE row set for all scenes + the rows' scene ids.  Returns
        [(bboxes, scores)] per scene, the levels concatenated: row for row what _get_bboxes_single gives for that scene alone
        (tests/test_head_select_gpu.py).  One scene: _cut_ids; several: _rank_by_scene, the runs sliced with the host counts.
        No plan flag is recorded."""
        nms_pre, per_scene = self.nms_pre, [([], []) for _ in range(n_scenes)]
        for cen, box, cls, pts, cs in self._fused_levels(centernesses, bbox_preds, cls_scores, points, scenes):
            if n_scenes == 1:
                groups = [_cut_ids(cls, cen, nms_pre)]
            else:
                counts = cs.batch_counts()                  # usually cached by the pruning step of the same level
                order = _rank_by_scene(cs.C[:, 0], S.max_scores(cls, cen))
                groups, r0 = [], 0
                for nb in counts:
                    groups.append(order[r0:r0 + nms_pre] if nb > nms_pre > 0 else torch.sort(order[r0:r0 + nb])[0])
                    r0 += nb
            for b, ids in enumerate(groups):
                self._decode_into(*per_scene[b], ids, cls, cen, box, pts)
        return [(torch.cat(bx), torch.cat(scr)) for bx, scr in per_scene]

    def loss(self, centernesses, bbox_preds, cls_scores, points, gt_bboxes, gt_labels):
        """per-scene assignment + centerness / IoU / focal losses, averaged over the scenes (reference :142-167)"""
        assert len(centernesses[0]) == len(bbox_preds[0]) == len(cls_scores[0]) == len(points[0]) == len(gt_bboxes) \
            == len(gt_labels)
        per = [self._loss_single([x[i] for x in centernesses], [x[i] for x in bbox_preds], [x[i] for x in cls_scores],
                                 [x[i] for x in points], gt_bboxes[i], gt_labels[i]) for i in range(len(gt_bboxes))]
        return dict(loss_centerness=torch.mean(torch.stack([p[0] for p in per])),
                    loss_bbox=torch.mean(torch.stack([p[1] for p in per])),
                    loss_cls=torch.mean(torch.stack([p[2] for p in per])))

    def _loss_single(self, centernesses, bbox_preds, cls_scores, points, gt_bboxes, gt_labels):
        """reference :170-214 (single process: reduce_mean is the identity; under DDP mmdet's reduce_mean averages the
        normalisers over the ranks)"""
        if self.assigner is None:
            raise ValueError("FCAF3DHead.loss needs an assigner (config key `assigner`)")
        if self.device_targets:
            return self._loss_single_device(centernesses, bbox_preds, cls_scores, points, gt_bboxes, gt_labels)
        if not hasattr(gt_bboxes, "gravity_center"):
            gt_bboxes = GTBoxes(torch.as_tensor(gt_bboxes))
        with torch.no_grad():
            centerness_targets, bbox_targets, labels = self.assigner.assign(points, gt_bboxes, gt_labels)
        centerness, bbox_pred, cls_score, pts = map(torch.cat, (centernesses, bbox_preds, cls_scores, points))
        pos = torch.nonzero(labels >= 0).squeeze(1)
        n_pos = max(_reduce_mean(torch.tensor(float(len(pos)), device=centerness.device)), 1.0)
        loss_cls = self.loss_cls(cls_score, labels, avg_factor=n_pos)
        pos_ctr, pos_box = centerness[pos], bbox_pred[pos]
        pos_ctr_t = centerness_targets[pos].unsqueeze(1)
        denorm = max(_reduce_mean(pos_ctr_t.sum().detach()), 1e-6)
        if len(pos) > 0:
            loss_centerness = self.loss_centerness(pos_ctr, pos_ctr_t, avg_factor=n_pos)
            loss_bbox = self.loss_bbox(self._bbox_pred_to_bbox(pts[pos], pos_box), bbox_targets[pos],
                                       weight=pos_ctr_t.squeeze(1), avg_factor=denorm)
        else:
            loss_centerness, loss_bbox = pos_ctr.sum(), pos_box.sum()
        return loss_centerness, loss_bbox, loss_cls


    def _loss_single_device(self, centernesses, bbox_preds, cls_scores, points, gt_bboxes, gt_labels):
        """_loss_single with the assignment and the three losses on the device (cnrma_amd.sparse.assign_targets /
        focal_loss_sum / positive_loss_sums): fixed shapes -- the ground truth padded to a multiple of 16 boxes, the positive
        rows in a block of m_cap * topk -- and device words for every count, so nothing is read back and the whole of it can be
        captured in a graph.  gt_bboxes may be a sparse.DeviceGT (already padded; gt_labels is then ignored).  No boxes at all
        is legal: loss_centerness = loss_bbox = 0 and the focal loss runs over all-background rows."""
        a = self.assigner
        if len(points) > a.n_scales:
            raise ValueError(f"{len(points)} levels for an assigner with n_scales={a.n_scales}")
        caps = [p.shape[0] for p in points] + [0] * (a.n_scales - len(points))     # a missing level holds no point
        centerness, bbox_pred, cls_score, pts = map(torch.cat, (centernesses, bbox_preds, cls_scores, points))
        dev = centerness.device
        if isinstance(gt_bboxes, S.DeviceGT):
            gt = gt_bboxes
        else:
            if not hasattr(gt_bboxes, "gravity_center"):
                gt_bboxes = GTBoxes(torch.as_tensor(gt_bboxes))
            gt = S.DeviceGT.from_boxes(gt_bboxes, gt_labels, dev)
        with torch.no_grad():
            labels, pos_row, pos_box, pos_ctr, n_pos = S.assign_targets(pts, caps, gt, a.limit, a.topk)
        focal = S.focal_loss_sum(cls_score, labels, caps, None, self.loss_cls.gamma, self.loss_cls.alpha)
        rows = pos_row.long()
        boxes = self._bbox_pred_to_bbox(pts.index_select(0, rows), bbox_pred.index_select(0, rows))
        rotated = bool(getattr(self.loss_bbox, "with_yaw", False)) and boxes.shape[1] >= 7
        sums = S.positive_loss_sums(centerness.index_select(0, rows), boxes, gt, pos_box, pos_ctr, n_pos, rotated)
        norm = _reduce_mean_device(torch.stack((n_pos[0].float(), sums[2].detach())))
        n_norm, ctr_norm = norm[0].clamp(min=1.0), norm[1].clamp(min=1e-6)
        return (self.loss_centerness.loss_weight * sums[0] / n_norm, self.loss_bbox.loss_weight * sums[1] / ctr_norm,
                self.loss_cls.loss_weight * focal / n_norm)


def _reduce_mean_device(t):
    """_reduce_mean that stays on the device: the normalisers averaged over the ranks as one tensor"""
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        t = t.clone()
        dist.all_reduce(t.div_(dist.get_world_size()))
    return t


def _reduce_mean(t):
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        t = t.clone()
        dist.all_reduce(t.div_(dist.get_world_size()))
    return float(t)


def compute_centerness(bbox_targets):
    """sqrt of the product over axes of min/max face distances (reference :395-402)."""
    d = bbox_targets[..., :6]
    x, y, z = d[..., 0:2], d[..., 2:4], d[..., 4:6]
    c = x.min(dim=-1)[0] / x.max(dim=-1)[0] * y.min(dim=-1)[0] / y.max(dim=-1)[0] * z.min(dim=-1)[0] / z.max(dim=-1)[0]
    return torch.sqrt(c)


@BBOX_ASSIGNERS.register_module()
class FCAF3DAssigner(object):
    """Point-to-box assignment of FCAF3D (reference :405-484): inside-box, best-scale (first level with fewer than
    `limit` inside points, minus one), top-k centerness, smallest volume."""

    def __init__(self, limit, topk, n_scales):
        self.limit, self.topk, self.n_scales = limit, topk, n_scales

    def assign(self, points, gt_bboxes, gt_labels):
        """points: list (per level) of [n_i,3]; gt_bboxes exposes .gravity_center [m,3], .tensor [m,7], .volume [m].
        Returns (centerness_targets [n], bbox_targets [n,7], labels [n], -1 = background)."""
        big = 1e8
        level = torch.cat([p.new_tensor(i).expand(len(p)) for i, p in enumerate(points)])
        pts = torch.cat(points, dim=0)
        n, m = len(pts), len(gt_bboxes)
        vol = gt_bboxes.volume.to(pts.device).expand(n, m).contiguous()
        box = torch.cat((gt_bboxes.gravity_center, gt_bboxes.tensor[:, 3:]), dim=1).to(pts.device)     # [m,7]
        boxes = box.expand(n, m, 7)
        rel = pts[:, None, :] - box[None, :, :3]                                                       # [n,m,3]
        # mmdet3d 0.15 rotation_3d_in_axis(shift, -yaw, axis=2): row-vector times [[c,-s,0],[s,c,0],[0,0,1]]
        # (third-party convention, not pinned by anything under /root/reference)
        ang = -box[:, 6]
        c, s = torch.cos(ang)[None], torch.sin(ang)[None]
        rot = torch.stack((rel[..., 0] * c + rel[..., 1] * s, -rel[..., 0] * s + rel[..., 1] * c, rel[..., 2]), dim=-1)
        centers = boxes[..., :3] + rot
        half = boxes[..., 3:6] / 2
        lo = centers - boxes[..., :3] + half                       # distances to the three "min" faces
        hi = boxes[..., :3] + half - centers                        # ... and the three "max" faces
        targets = torch.stack((lo[..., 0], hi[..., 0], lo[..., 1], hi[..., 1], lo[..., 2], hi[..., 2], boxes[..., 6]), -1)
        inside = targets[..., :6].min(-1)[0] > 0                                                     # condition 1
        per_level = torch.stack([inside[level == i].sum(dim=0) for i in range(self.n_scales)], dim=0)  # [L,m]
        too_few = per_level < self.limit
        lower = torch.argmax(too_few.int(), dim=0) - 1
        lower = torch.where(lower < 0, torch.zeros_like(lower), lower)
        best = torch.where(torch.all(~too_few, dim=0), torch.full_like(lower, self.n_scales - 1), lower)
        at_best = best[None, :].expand(n, m) == level[:, None].expand(n, m)                           # condition 2
        cness = compute_centerness(targets)
        cness = torch.where(inside & at_best, cness, -torch.ones_like(cness))
        kth = torch.topk(cness, min(self.topk + 1, len(cness)), dim=0).values[-1]
        top = cness > kth[None]                                                                       # condition 3
        vol = torch.where(inside & at_best & top, vol, torch.full_like(vol, big))
        min_vol, arg = vol.min(dim=1)
        labels = torch.where(min_vol == big, torch.full_like(gt_labels[arg], -1), gt_labels[arg])
        rows = torch.arange(n, device=pts.device)
        picked = targets[rows, arg]
        return compute_centerness(picked), boxes[rows, arg], labels
