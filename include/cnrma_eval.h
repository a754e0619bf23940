/*
 * cnrma_eval.h -- C-ABI of libcnrma_eval_hip.so: the indoor mAP evaluation of CN-RMA's detections on the MI355X (gfx950).
 *
 * A library of its own beside libcnrma_hip.so (include/cnrma.h) and libcnrma_prep_hip.so (include/cnrma_prep.h).  The conventions
 * are cnrma.h's: every pointer is a DEVICE pointer, buffers are caller-owned, the library never allocates, frees or synchronises,
 * `stream` is a hipStream_t passed as void*, 0 = ok, negative = -(hipError_t) of a failed launch or CNRMA_EVAL_EINVAL for bad
 * arguments (answered before any launch); re-entrant, no global mutable state, nothing read from the environment.
 *
 * What is computed is mmdet3d's indoor_eval (eval_det_cls / eval_map_recall) as cnrma_amd.postprocess.indoor_eval restates it,
 * decision for decision; the reference's call site is post_process/evaluate_bbox.py:93-100.
 */
#ifndef CNRMA_EVAL_H
#define CNRMA_EVAL_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CNRMA_EVAL_EINVAL (-22)
#define CNRMA_EVAL_ABI_VERSION 1

int cnrma_eval_abi_version(void);

/* ------------------------------------------------------------------------------------------------------------
 * e1  The accumulator: detections and ground truth of many scenes in flat, capacity-sized arrays
 *     det_boxes [det_cap][7] f32, det_scores [det_cap] f32, det_labels [det_cap] i32, det_scene [det_cap] i32 (scene of the row)
 *     gt_boxes  [gt_cap][7]  f32, gt_labels  [gt_cap]  i32
 *     scene_gt  [scene_cap][2] i32: the rows [begin, end) of gt_boxes that belong to the scene, clamped to gt_cap
 *     counters  [4] i32: detections, ground-truth boxes and scenes appended so far -- the TRUE totals, which keep counting when
 *               rows no longer fit (a total above its capacity = overflow, found when the caller reads the counters) --, and 0.
 * cnrma_eval_reset: counters = 0.
 * cnrma_eval_append_f32: one scene.  boxes [n_rows][box_cols], scores [n_rows], labels [n_rows] (label_bytes = 4: int32,
 *   8: int64) are a padded block whose first min(n_rows, max(*n_live, 0)) rows are live (n_live NULL: all of them); dead rows are
 *   never read.  gt_boxes [n_gt][gt_cols], gt_labels [n_gt] (gt_label_bytes as above).  box_cols / gt_cols 6 or 7; six columns
 *   get heading 0.  Live rows go behind the cursors; rows that do not fit (and every row of a scene beyond scene_cap) are
 *   dropped, nothing is written past a capacity.  ONE launch of one workgroup, nothing read back: capturable; appends on one
 *   stream are ordered by the stream.
 * Returns -22 for a negative count or capacity, box_cols / gt_cols not 6 or 7, label_bytes not 4 or 8, a NULL state pointer, or
 *   a NULL input of a non-empty block.
 * ---------------------------------------------------------------------------------------------------------- */
int cnrma_eval_reset(int32_t* counters, void* stream);
int cnrma_eval_append_f32(const float* boxes, int box_cols, const float* scores, const void* labels, int label_bytes, int n_rows,
                          const int32_t* n_live, const float* gt_boxes, int gt_cols, const void* gt_labels, int gt_label_bytes,
                          int n_gt, float* st_det_boxes, float* st_det_scores, int32_t* st_det_labels, int32_t* st_det_scene,
                          int det_cap, float* st_gt_boxes, int32_t* st_gt_labels, int gt_cap, int32_t* st_scene_gt, int scene_cap,
                          int32_t* counters, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * e2  Matching and AP over everything appended: best box, claim, flag, AP -- five launches whatever the number of scenes
 * n_det, n_gt, n_scenes: the rows in use (the caller read the counters).  order [n_det] int64: the detections sorted by
 * (label ascending, score descending, row ascending).  thresholds [T] f32, each in [0, 1); T in 1 .. 8.
 *   best    detection i scans the boxes of its scene (scene_gt) with its label, in row order: best_iou[i] = the largest 3D IoU
 *           (BEV overlap x height overlap; `rotated` != 0: polygon clipping, else axis-aligned -- cnrma_box_iou_f32's arithmetic
 *           with mode3d = 1, bit for bit), best_gt[i] = the FIRST row that reaches it; no such box: 0 and -1.
 *   claim   for every t, the detection at sorted position p with best_iou > thresholds[t] (strict, fp32) does
 *           claim[t][best_gt] = min(claim[t][best_gt], p): an unsigned minimum, independent of the order of arrival.
 *   flag    flags[i] bit t = (best_iou > thresholds[t] and claim[t][best_gt] == p): the first detection in score order among
 *           those that chose the box and pass the threshold is the true positive.  flags [n_det] uint8, in row order.
 *   ap      per (t, class c): the detections with label c in sorted order, ctp = inclusive count of true positives,
 *           prec_k = ctp_k / (k + 1), env_k = max over k' >= k of prec_k', ap = sum over the true positives of
 *           (ctp_k / n_gt - (ctp_k - 1) / n_gt) * env_k, recall = ctp_last / n_gt; all float64.
 * table [T][n_classes][4] f64: ap, recall, n_gt (boxes with label c), n_det (detections with label c); n_gt == 0: ap = recall = 0.
 * Scores and boxes are taken to be finite; nothing checks it.
 * cnrma_eval_result_workspace_bytes: bytes of `workspace` (16-byte aligned); 0 for arguments the call would refuse.
 * Returns -22 for a negative count, T outside 1 .. 8, n_classes < 1, a short workspace or a NULL required pointer (table,
 *   thresholds, workspace always; the detection arrays, order and the outputs when n_det > 0; the ground-truth arrays when
 *   n_gt > 0; scene_gt when n_det > 0).
 * ---------------------------------------------------------------------------------------------------------- */
size_t cnrma_eval_result_workspace_bytes(int n_det, int n_gt, int T);
int cnrma_eval_result_f32(const float* det_boxes, const int32_t* det_labels, const int32_t* det_scene, int n_det,
                          const float* gt_boxes, const int32_t* gt_labels, int n_gt, const int32_t* scene_gt, int n_scenes,
                          int rotated, const int64_t* order, const float* thresholds, int T, int n_classes, void* workspace,
                          size_t workspace_bytes, float* best_iou, int32_t* best_gt, uint8_t* flags, double* table,
                          void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CNRMA_EVAL_H */
