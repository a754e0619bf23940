"""Indoor mAP on the device (include/cnrma_eval.h, csrc/eval.hip): postprocess.indoor_eval -- mmdet3d's eval_det_cls /
eval_map_recall -- for all scenes, classes and thresholds in one pass, decision for decision.

    ev = DetectionEvaluator(n_classes=18)
    ev.add(boxes, scores, labels, gt_boxes, gt_labels, n=n_out)      # per scene; padded form: no host read, capturable
    ev.result()                                                      # {"mAP_0.25": .., "mAR_0.25": .., "AP_0.25": [..], ..}

The detections and the ground truth of every added scene live in flat, capacity-sized device arrays behind device-side cursors.
result() orders the detections (two stable torch sorts) and calls cnrma_eval_result_f32: best box, claim, flag, AP -- five
launches whatever the number of scenes --, with two device->host reads: the cursors, then the [T][n_classes] table.
Scores and boxes are taken to be finite: nothing on the device checks it."""
import numpy as np
import torch

from . import _lib
from ._lib import CnrmaError, call_eval, ptr, stream

MAX_THRESHOLDS = 8


def _layout(det_cap, gt_cap, scene_cap):
    """name -> (first int32 word, words) of the evaluator's state block; float arrays are views of the same words"""
    out, at = {}, 0
    for name, words in (("counters", 4), ("scene_gt", 2 * scene_cap), ("det_labels", det_cap), ("det_scene", det_cap),
                        ("gt_labels", gt_cap), ("det_scores", det_cap), ("det_boxes", 7 * det_cap), ("gt_boxes", 7 * gt_cap)):
        out[name] = (at, words)
        at += words
    return out, at


_FLOAT_FIELDS = ("det_scores", "det_boxes", "gt_boxes")


class DetectionEvaluator:
    """Accumulates scenes on the device and evaluates them like postprocess.indoor_eval.

    rotated: the IoU of the whole evaluation -- polygon clipping (True) or axis-aligned (False).  indoor_eval decides it per
    call from the column count (7 columns on either side: rotated); seven-column boxes need rotated=True here.  Within one
    evaluation every detection block has one column count and every ground-truth block has one; six columns get heading 0.
    The capacities bound what add() may append; result() raises when a total exceeds its capacity."""

    def __init__(self, n_classes, iou_thrs=(0.25, 0.5), rotated=False, det_capacity=1 << 18, gt_capacity=1 << 16,
                 scene_capacity=4096, device="cuda"):
        iou_thrs = tuple(float(t) for t in iou_thrs)
        if int(n_classes) < 1:
            raise ValueError(f"n_classes must be >= 1 (got {n_classes})")
        if not 1 <= len(iou_thrs) <= MAX_THRESHOLDS or not all(0.0 <= t < 1.0 for t in iou_thrs):
            raise ValueError(f"1 to {MAX_THRESHOLDS} IoU thresholds, each in [0, 1) (got {iou_thrs})")
        if min(int(det_capacity), int(gt_capacity), int(scene_capacity)) < 1:
            raise ValueError("det_capacity, gt_capacity and scene_capacity must be >= 1")
        _lib.require_gpu()
        self.n_classes, self.iou_thrs, self.rotated = int(n_classes), iou_thrs, bool(rotated)
        self.det_capacity, self.gt_capacity, self.scene_capacity = int(det_capacity), int(gt_capacity), int(scene_capacity)
        self.device = torch.device(device)
        self._fields, words = _layout(self.det_capacity, self.gt_capacity, self.scene_capacity)
        self._state = torch.zeros(words, dtype=torch.int32, device=self.device)
        for name, (at, n) in self._fields.items():
            view = self._state[at:at + n]
            setattr(self, "_" + name, view.view(torch.float32) if name in _FLOAT_FIELDS else view)
        self._thresholds = torch.tensor(iou_thrs, dtype=torch.float32, device=self.device)
        self._cols = {"detections": None, "ground truth": None}

    def reset(self):
        """forget every added scene (one launch; the arrays keep their capacity)"""
        call_eval("cnrma_eval_reset", ptr(self._counters), stream())
        self._cols = {"detections": None, "ground truth": None}

    def _check_cols(self, what, cols):
        if cols not in (6, 7):
            raise ValueError(f"{what}: boxes have 6 or 7 columns (got {cols})")
        if cols == 7 and not self.rotated:
            raise ValueError(f"{what} carry a heading (7 columns): construct the evaluator with rotated=True")
        if self._cols[what] not in (None, cols):
            raise ValueError(f"{what}: scenes with {self._cols[what]} and with {cols} columns in one evaluation")
        self._cols[what] = cols

    def _boxes(self, what, boxes):
        boxes = torch.as_tensor(boxes).to(self.device, torch.float32)
        if boxes.numel() == 0:                                           # no rows: the column count says nothing
            return boxes.reshape(0, 6)
        if boxes.ndim != 2:
            raise ValueError(f"{what}: boxes must be [n, 6|7] (got {tuple(boxes.shape)})")
        self._check_cols(what, boxes.shape[1])
        return boxes.contiguous()

    def _labels(self, labels, rows):
        labels = torch.as_tensor(labels).to(self.device)
        if labels.dtype not in (torch.int32, torch.int64):
            labels = labels.to(torch.int64)
        labels = labels.reshape(-1).contiguous()
        if labels.numel() != rows:
            raise ValueError(f"{labels.numel()} labels for {rows} boxes")
        return labels

    def add(self, boxes, scores, labels, gt_boxes, gt_labels, n=None):
        """one scene: detections (boxes [k, 6|7], scores [k], labels [k]) and ground truth (gt_boxes [g, 6|7], gt_labels [g]).
        Device tensors are taken as they are, host arrays are uploaded.  n=None: every row is live.  n = a device int32 [1]:
        the detections are a padded block whose first n rows are live -- what nms_device(padded=True) returns; dead rows are
        never read, nothing is read back, and the call can be captured (a plain single-stream region)."""
        boxes, gt_boxes = self._boxes("detections", boxes), self._boxes("ground truth", gt_boxes)
        scores = torch.as_tensor(scores).to(self.device, torch.float32).reshape(-1).contiguous()
        if scores.numel() != boxes.shape[0]:
            raise ValueError(f"{scores.numel()} scores for {boxes.shape[0]} boxes")
        labels, gt_labels = self._labels(labels, boxes.shape[0]), self._labels(gt_labels, gt_boxes.shape[0])
        if n is not None:
            if not (torch.is_tensor(n) and n.is_cuda and n.dtype == torch.int32 and n.numel() == 1):
                raise ValueError("n must be a device int32 tensor with one element (or None)")
        call_eval("cnrma_eval_append_f32", ptr(boxes), boxes.shape[1], ptr(scores), ptr(labels), labels.element_size(),
                  boxes.shape[0], ptr(n), ptr(gt_boxes), gt_boxes.shape[1], ptr(gt_labels), gt_labels.element_size(),
                  gt_boxes.shape[0], ptr(self._det_boxes), ptr(self._det_scores), ptr(self._det_labels), ptr(self._det_scene),
                  self.det_capacity, ptr(self._gt_boxes), ptr(self._gt_labels), self.gt_capacity, ptr(self._scene_gt),
                  self.scene_capacity, ptr(self._counters), stream())

    def result(self, return_flags=False):
        """the dict of postprocess.indoor_eval over everything added.  return_flags=True: (dict, flags) with flags =
        dict(best_iou float32 [n], best_gt int32 [n] (row among all added ground-truth boxes, -1: none), tp uint8 [n] (bit t:
        true positive at iou_thrs[t]) -- device tensors in the order the detections were added --, n_gt and n_det per class)."""
        n_det, n_gt, n_scenes = _lib.read_ints(self._counters)[:3]                         # read 1: the cursors
        for total, cap, name in ((n_det, self.det_capacity, "det_capacity"), (n_gt, self.gt_capacity, "gt_capacity"),
                                 (n_scenes, self.scene_capacity, "scene_capacity")):
            if total > cap:
                raise CnrmaError(f"{name}={cap} is too small: {total} rows were added (rows beyond the capacity were dropped); "
                                 f"build the evaluator with a larger {name}")
        by_score = torch.sort(self._det_scores[:n_det], descending=True, stable=True).indices
        by_label = torch.sort(self._det_labels[:n_det][by_score], stable=True).indices
        order = by_score[by_label].contiguous()               # (label ascending, score descending, row ascending)
        T = len(self.iou_thrs)
        ws = torch.empty(_lib.load_eval().cnrma_eval_result_workspace_bytes(n_det, n_gt, T), dtype=torch.uint8, device=self.device)
        best_iou = torch.empty(n_det, dtype=torch.float32, device=self.device)
        best_gt = torch.empty(n_det, dtype=torch.int32, device=self.device)
        tp = torch.empty(n_det, dtype=torch.uint8, device=self.device)
        table = torch.empty((T, self.n_classes, 4), dtype=torch.float64, device=self.device)
        call_eval("cnrma_eval_result_f32", ptr(self._det_boxes), ptr(self._det_labels), ptr(self._det_scene), n_det,
                  ptr(self._gt_boxes), ptr(self._gt_labels), n_gt, ptr(self._scene_gt), n_scenes, int(self.rotated), ptr(order),
                  ptr(self._thresholds), T, self.n_classes, ptr(ws), ws.numel(), ptr(best_iou), ptr(best_gt), ptr(tp),
                  ptr(table), stream())
        tab = table.cpu().numpy()                                                          # read 2: the table
        result = {}
        for t, thr in enumerate(self.iou_thrs):
            counted = tab[t, :, 2] > 0                        # a class without ground truth is left out, as in indoor_eval
            aps, recs = [float(v) for v in tab[t, counted, 0]], [float(v) for v in tab[t, counted, 1]]
            result[f"mAP_{thr:.2f}"] = float(np.mean(aps)) if aps else 0.0
            result[f"mAR_{thr:.2f}"] = float(np.mean(recs)) if recs else 0.0
            result[f"AP_{thr:.2f}"] = aps
        if not return_flags:
            return result
        return result, dict(best_iou=best_iou, best_gt=best_gt, tp=tp, n_gt=tab[0, :, 2].astype(np.int64),
                            n_det=tab[0, :, 3].astype(np.int64))


def _host_boxes(what, blocks):
    """the scenes' box arrays as float32 [k, 6|7] with ONE column count (empty blocks take it from the others)"""
    blocks = [np.asarray(b, dtype=np.float32) for b in blocks]
    cols = {b.shape[1] for b in blocks if b.ndim == 2 and b.shape[0]}
    if len(cols) > 1 or not cols <= {6, 7} or any(b.ndim != 2 for b in blocks if b.size):
        raise ValueError(f"{what}: every scene's boxes must be [k, 6] or every scene's [k, 7] (column counts {sorted(cols)})")
    c = cols.pop() if cols else 6
    return [b if b.size else b.reshape(0, c) for b in blocks], c


def _host_labels(labels):
    labels = np.asarray(labels).astype(np.int64).reshape(-1)
    return np.where((labels < -2 ** 31) | (labels >= 2 ** 31), -1, labels).astype(np.int32)


def indoor_eval_device(gt_annos, dt_annos, iou_thrs=(0.25, 0.5), n_classes=None, device="cuda"):
    """postprocess.indoor_eval -- same arguments, same dict -- through one DetectionEvaluator: the scenes are concatenated on
    the host into the evaluator's state layout and uploaded in ONE copy; then result().  The IoU is rotated iff the detections
    or the ground truth carry 7 columns; scenes whose column counts differ are a ValueError."""
    pairs = list(zip(gt_annos, dt_annos))
    if n_classes is None:
        n_classes = 1 + max([int(np.max(g["labels"])) for g, _ in pairs if len(g["labels"])] +
                            [int(np.max(d["labels"])) for _, d in pairs if len(d["labels"])] + [0])
    db, dcols = _host_boxes("detections", [d["boxes"] for _, d in pairs])
    gb, gcols = _host_boxes("ground truth", [g["boxes"] for g, _ in pairs])
    ds = [np.asarray(d["scores"], dtype=np.float32).reshape(-1) for _, d in pairs]
    dl, gl = [_host_labels(d["labels"]) for _, d in pairs], [_host_labels(g["labels"]) for g, _ in pairs]
    for k, (b, s, l, g, m) in enumerate(zip(db, ds, dl, gb, gl)):
        if not len(b) == len(s) == len(l) or len(g) != len(m):
            raise ValueError(f"scene {k}: boxes, scores and labels differ in length")
    n_det, n_gt, n_scenes = sum(map(len, db)), sum(map(len, gb)), len(pairs)
    ev = DetectionEvaluator(n_classes, iou_thrs, rotated=dcols == 7 or gcols == 7, det_capacity=max(n_det, 1),
                            gt_capacity=max(n_gt, 1), scene_capacity=max(n_scenes, 1), device=device)
    fields, words = _layout(ev.det_capacity, ev.gt_capacity, ev.scene_capacity)
    blob = np.zeros(words, dtype=np.int32)

    def put(name, values):
        values = np.ascontiguousarray(values).reshape(-1)
        blob[fields[name][0]:fields[name][0] + values.size] = values.view(np.int32)

    def boxes7(blocks, cols, rows):
        out = np.zeros((rows, 7), dtype=np.float32)
        if rows:
            out[:, :cols] = np.concatenate(blocks)
        return out
    gt_end = np.cumsum([len(g) for g in gb], dtype=np.int64).astype(np.int32)
    put("counters", np.array([n_det, n_gt, n_scenes, 0], dtype=np.int32))
    put("scene_gt", np.stack((gt_end - np.array([len(g) for g in gb], dtype=np.int32), gt_end), axis=1).astype(np.int32)
        if n_scenes else np.zeros(0, np.int32))
    if n_det:
        put("det_labels", np.concatenate(dl))
        put("det_scene", np.repeat(np.arange(n_scenes, dtype=np.int32), [len(b) for b in db]))
        put("det_scores", np.concatenate(ds))
    if n_gt:
        put("gt_labels", np.concatenate(gl))
    put("det_boxes", boxes7(db, dcols, n_det))
    put("gt_boxes", boxes7(gb, gcols, n_gt))
    ev._state.copy_(torch.from_numpy(blob))                   # the one upload
    return ev.result()
