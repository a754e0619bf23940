"""The device mAP evaluation (cnrma_amd.evaluate, csrc/eval.hip) against the host evaluator postprocess.indoor_eval -- same IoU
arithmetic, so every discrete result must be EQUAL and nothing is excluded -- and against the float64 oracle tests/eval_oracle.py,
which shares no clipping code with the kernels.

AP / recall bound 1e-9: derived, not measured.  Flags being equal, the only freedom is the order of the float64 sum of at most
n_gt positive terms that add up to at most 1: an error of at most n_gt * 2^-53, below 1.2e-10 for a million boxes."""
import ast
import functools
import os
import runpy
import sys

import numpy as np
import pytest
import torch

import eval_oracle as EO

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AP_TOL = 1e-9
T8 = (0.0, 0.125, 0.25, 0.375, 0.5, 0.625, 0.75, 0.875)          # all exact in float32
GUARD = -7777


def host_reference(gts, dts, thrs, n_classes, dev):
    """indoor_eval's own loop (box_iou per class and scene, argmax, `used`), keeping what it throws away: per detection, in the
    order given, the row maximum of the IoU matrix (float32), its argmax as a row among ALL ground-truth boxes, and the
    true-positive bits; plus indoor_eval's dict and n_gt per class"""
    from cnrma_amd import postprocess as PP
    rot = any(np.asarray(a["boxes"]).shape[-1] == 7 for a in list(gts) + list(dts) if len(a["labels"]))
    best_iou, best_gt, tp, off = [], [], [], 0
    for g, d in zip(gts, dts):
        n = len(d["labels"])
        bi, bg, bits = np.zeros(n, np.float32), np.full(n, -1, np.int32), np.zeros(n, np.uint8)
        for c in range(n_classes):
            gi, di = np.nonzero(np.asarray(g["labels"]) == c)[0], np.nonzero(np.asarray(d["labels"]) == c)[0]
            if len(gi) == 0 or len(di) == 0:
                continue
            order = di[np.argsort(-np.asarray(d["scores"], np.float32)[di], kind="stable")]
            iou = PP.box_iou(torch.from_numpy(np.asarray(d["boxes"], np.float32)[order]).to(dev),
                             torch.from_numpy(np.asarray(g["boxes"], np.float32)[gi]).to(dev), rotated=rot, mode3d=True).cpu().numpy()
            bi[order], bg[order] = iou.max(axis=1), off + gi[iou.argmax(axis=1)]
            for t, thr in enumerate(thrs):
                used = np.zeros(len(gi), dtype=bool)
                for r, i in enumerate(order):
                    j = int(np.argmax(iou[r]))
                    if iou[r, j] > thr and not used[j]:
                        bits[i] |= np.uint8(1 << t)
                        used[j] = True
        best_iou.append(bi), best_gt.append(bg), tp.append(bits)
        off += len(g["labels"])
    cat = lambda xs, dt: np.concatenate(xs).astype(dt) if xs else np.zeros(0, dt)
    n_gt = np.array([sum(int(np.sum(np.asarray(g["labels"]) == c)) for g in gts) for c in range(n_classes)])
    return dict(best_iou=cat(best_iou, np.float32), best_gt=cat(best_gt, np.int32), tp=cat(tp, np.uint8), n_gt=n_gt,
                result=PP.indoor_eval(gts, dts, thrs, n_classes=n_classes, device=dev))


def assert_same_dict(got, exp):
    assert list(got) == list(exp)
    for k in exp:
        if k.startswith("AP_"):
            assert len(got[k]) == len(exp[k]), k
        print(k, got[k], exp[k])
        np.testing.assert_allclose(np.asarray(got[k], np.float64), np.asarray(exp[k], np.float64), rtol=0, atol=AP_TOL, err_msg=k)


def assert_same_flags(flags, ref):
    assert np.array_equal(flags["best_gt"].cpu().numpy(), ref["best_gt"])
    assert np.array_equal(flags["best_iou"].cpu().numpy().view(np.uint32), ref["best_iou"].view(np.uint32))      # bit for bit
    assert np.array_equal(flags["tp"].cpu().numpy(), ref["tp"])
    assert np.array_equal(flags["n_gt"], ref["n_gt"])


def evaluator_for(gts, dts, thrs, n_classes, dev, **kw):
    from cnrma_amd.evaluate import DetectionEvaluator
    rot = any(np.asarray(a["boxes"]).shape[-1] == 7 for a in list(gts) + list(dts) if len(a["labels"]))
    kw = dict(dict(det_capacity=max(1, sum(len(d["labels"]) for d in dts)), gt_capacity=max(1, sum(len(g["labels"]) for g in gts)),
                   scene_capacity=max(1, len(gts))), **kw)
    return DetectionEvaluator(n_classes, thrs, rotated=rot, device=dev, **kw)


def add_all(ev, gts, dts):
    for g, d in zip(gts, dts):
        ev.add(d["boxes"], d["scores"], d["labels"], g["boxes"], g["labels"])
    return ev


@functools.lru_cache(maxsize=None)
def dataset(seed, det_cols, gt_cols, regular, thrs, duplicates=True):
    """the data set and its host reference, computed once and shared (never written to)"""
    gts, dts, n_classes = EO.make_dataset(seed, det_cols, gt_cols, regular=regular, duplicates=duplicates)
    return gts, dts, n_classes, host_reference(gts, dts, thrs, n_classes, torch.device("cuda:0"))


# ---- exact against the host evaluator ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("thrs", [(0.25, 0.5), (0.125, 0.75)])
@pytest.mark.parametrize("det_cols,gt_cols,regular", [(6, 6, 3), (7, 7, 3), (7, 6, 3), (6, 7, 3), (6, 6, 1), (7, 7, 1)])
def test_equals_the_host_evaluator(device, det_cols, gt_cols, regular, thrs):
    from cnrma_amd import postprocess as PP
    gts, dts, n_classes, ref = dataset(1, det_cols, gt_cols, regular, thrs)
    assert (ref["tp"] != 0).sum() >= 10 and len(set(ref["tp"].tolist())) >= 2          # the thresholds tell detections apart
    res, flags = add_all(evaluator_for(gts, dts, thrs, n_classes, device), gts, dts).result(return_flags=True)
    assert_same_flags(flags, ref)
    assert_same_dict(res, ref["result"])
    assert len(res[f"AP_{thrs[0]:.2f}"]) == int((ref["n_gt"] > 0).sum()) == n_classes - 1
    assert_same_dict(PP.indoor_eval_device(gts, dts, thrs, n_classes=n_classes, device=device), ref["result"])
    assert_same_dict(PP.indoor_eval_device(gts, dts, thrs, device=device), PP.indoor_eval(gts, dts, thrs, device=device))


def test_identical_boxes_keep_the_argmax_quirk(device):
    gts, dts, n_classes, ref = dataset(1, 7, 7, 3, (0.25, 0.5))
    first = sum(len(d["labels"]) for d in dts[:10])
    d = dts[10]
    i, j = [(i, j) for i in range(len(d["labels"])) for j in range(i) if (d["boxes"][i] == d["boxes"][j]).all()][0]
    gt0 = sum(len(g["labels"]) for g in gts[:10])
    _, flags = add_all(evaluator_for(gts, dts, (0.25, 0.5), n_classes, device), gts, dts).result(return_flags=True)
    tp, bg = flags["tp"].cpu().numpy(), flags["best_gt"].cpu().numpy()
    assert bg[first + i] == bg[first + j] == gt0 and not (bg == gt0 + 1).any()       # the second of the identical boxes is never named
    assert int(tp[first + i]) & int(tp[first + j]) == 0                              # so at most one of the two is a true positive
    assert np.array_equal(tp, ref["tp"])


# ---- against the float64 oracle ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("det_cols,gt_cols,seed", [(6, 6, 0), (6, 6, 3), (7, 7, 0), (7, 7, 6)])
def test_equals_the_float64_oracle(device, det_cols, gt_cols, seed):
    thrs = (0.25, 0.5)
    gts, dts, n_classes = EO.make_dataset(seed, det_cols, gt_cols, duplicates=False)
    exp, scenes = EO.evaluate(gts, dts, thrs, n_classes)
    # conditions on the INPUT, checked on the oracle alone: the kernels agree with the oracle's IoU to 2e-5, so beyond 1e-4 of a
    # threshold, and with the two best boxes 1e-4 apart, float32 decides as float64 does.  No case is left out.
    to_threshold, gap = EO.margins(scenes, thrs)
    assert to_threshold > 1e-4 and gap > 1e-4
    res, flags = add_all(evaluator_for(gts, dts, thrs, n_classes, device), gts, dts).result(return_flags=True)
    tp = np.concatenate([m["tp"] for m in scenes])
    assert tp.any(axis=0).all() and not tp.all(axis=0).any()
    assert np.array_equal(flags["tp"].cpu().numpy(), (tp * (1 << np.arange(len(thrs)))).sum(axis=1).astype(np.uint8))
    assert_same_dict(res, exp)


# ---- edge sizes ----------------------------------------------------------------------------------------------------------------------
def one_scene(seed, n_det, n_gt, cols=7, n_classes=2):
    rng = np.random.default_rng(seed)
    gb = EO.random_boxes(rng, n_gt, cols, extent=max(1.5, 0.6 * n_gt ** 0.5))
    gl = rng.integers(0, n_classes, n_gt)
    src = rng.integers(0, n_gt, n_det)
    dl = np.where(rng.random(n_det) < 0.9, gl[src], rng.integers(0, n_classes, n_det))
    return (dict(boxes=gb, labels=gl.astype(np.int64)),
            dict(boxes=EO.jitter(rng, gb[src], cols), scores=EO.quantised_scores(rng, n_det), labels=dl.astype(np.int64)))


def check_against_host(device, gts, dts, thrs, n_classes):
    ref = host_reference(gts, dts, thrs, n_classes, device)
    res, flags = add_all(evaluator_for(gts, dts, thrs, n_classes, device), gts, dts).result(return_flags=True)
    assert_same_flags(flags, ref)
    assert_same_dict(res, ref["result"])
    return ref


@pytest.mark.parametrize("n_gt", [1, 64, 65])
@pytest.mark.parametrize("n_det", [1, 63, 64, 65, 255, 256, 257])
def test_edge_counts(device, n_det, n_gt):
    g, d = one_scene(n_det * 100 + n_gt, n_det, n_gt)
    ref = check_against_host(device, [g], [d], (0.25, 0.5), 2)
    assert n_det < 63 or ref["tp"].any()


def test_two_scenes_across_wave_and_block_boundaries(device):
    """60 + 200 detections: the second scene begins inside the first wave and runs across the 64-lane tiles and the 256-thread block
    of the best-box kernel; the scenes' ground-truth ranges differ (5 and 9 boxes)"""
    (g0, d0), (g1, d1) = one_scene(5, 60, 5), one_scene(6, 200, 9)
    ref = check_against_host(device, [g0, g1], [d0, d1], (0.25, 0.5), 2)
    assert ref["best_gt"][:60].max() < 5 <= ref["best_gt"][60:][ref["best_gt"][60:] >= 0].min() and ref["tp"].any()


@pytest.mark.parametrize("thrs", [(0.25,), T8])
def test_one_and_eight_thresholds(device, thrs):
    (g0, d0), (g1, d1) = one_scene(7, 90, 12), one_scene(8, 70, 7)
    ref = check_against_host(device, [g0, g1], [d0, d1], thrs, 2)
    assert len(set(ref["tp"].tolist())) >= (2 if len(thrs) == 1 else 5)


def test_one_class(device):
    g, d = one_scene(9, 130, 20, cols=6, n_classes=1)
    check_against_host(device, [g], [d], (0.25, 0.5), 1)


# ---- the accumulator -------------------------------------------------------------------------------------------------------------------
def guarded(t, keep):
    """a copy of `t` inside an allocation of its own with 8 guard elements on either side"""
    buf = torch.full((t.numel() + 16,), GUARD, dtype=t.dtype, device=t.device)
    keep.append(buf)
    view = buf[8:8 + t.numel()]
    view.copy_(t.reshape(-1))
    return view.view(t.shape)


def guards_intact(keep):
    return all(bool((b[:8] == GUARD).all()) and bool((b[-8:] == GUARD).all()) for b in keep)


def guard_state(ev, keep):
    for name in ev._fields:
        setattr(ev, "_" + name, guarded(getattr(ev, "_" + name), keep))
    return ev


def padded_scene(g, d, rows, live, dev, keep):
    """the scene as device tensors: detections in a block of `rows` rows whose rows behind `live` are poisoned"""
    cols = d["boxes"].shape[1]
    b, s = torch.full((rows, cols), float("nan")), torch.full((rows,), float("nan"))
    l = torch.full((rows,), 1 << 40, dtype=torch.int64)
    b[:live], s[:live], l[:live] = (torch.from_numpy(d[k][:live]) for k in ("boxes", "scores", "labels"))
    dev_t = lambda t: guarded(t.to(dev), keep)
    return dict(boxes=dev_t(b), scores=dev_t(s), labels=dev_t(l), gt_boxes=dev_t(torch.from_numpy(g["boxes"])),
                gt_labels=dev_t(torch.from_numpy(g["labels"])), n=dev_t(torch.tensor([live], dtype=torch.int32)))


def test_padded_add_reads_no_dead_row_and_writes_nowhere_else(device):
    """device n = 0, 1 and the full block; dead rows NaN (labels 2^40), -7777 around every input and every state buffer"""
    scenes = [one_scene(20 + k, 70, 6) for k in range(3)]
    gts, dts = [g for g, _ in scenes], [dict(d) for _, d in scenes]
    live = [0, 1, 70]
    for d, n in zip(dts, live):
        for k in ("boxes", "scores", "labels"):
            d[k] = d[k][:n]
    keep = []
    ev = guard_state(evaluator_for(gts, dts, (0.25, 0.5), 2, device), keep)
    for (g, d), n in zip(scenes, live):
        ev.add(**padded_scene(g, d, 70, n, device, keep))
    res, flags = ev.result(return_flags=True)
    torch.cuda.synchronize()
    assert guards_intact(keep)
    exp_res, exp = add_all(evaluator_for(gts, dts, (0.25, 0.5), 2, device), gts, dts).result(return_flags=True)
    assert flags["tp"].numel() == 71 and exp["tp"].any()
    for k in ("best_iou", "best_gt", "tp"):
        assert torch.equal(flags[k], exp[k])
    assert res == exp_res
    assert_same_flags(flags, host_reference(gts, dts, (0.25, 0.5), 2, device))


def test_padded_add_does_not_synchronise(device):
    g, d = one_scene(30, 40, 5)
    ev = evaluator_for([g], [d], (0.25, 0.5), 2, device)
    block = padded_scene(g, d, 64, 40, device, [])
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        ev.add(**block)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert ev.result() == add_all(evaluator_for([g], [d], (0.25, 0.5), 2, device), [g], [d]).result()


def test_replayed_capture_equals_eager_adds(device):
    """one captured add, replayed for three scenes whose contents are copied into the static buffers"""
    scenes, live, keep = [one_scene(40 + k, 48, 6) for k in range(3)], [48, 1, 17], []
    blocks = [padded_scene(g, d, 48, n, device, keep) for (g, d), n in zip(scenes, live)]
    gts, dts = [g for g, _ in scenes], [d for _, d in scenes]
    eager = evaluator_for(gts, dts, (0.25, 0.5), 2, device)
    for b in blocks:
        eager.add(**b)
    exp_res, exp = eager.result(return_flags=True)
    ev = evaluator_for(gts, dts, (0.25, 0.5), 2, device)
    static = {k: v.clone() for k, v in blocks[0].items()}
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ev.add(**static)
    for b in blocks:
        for k in static:
            static[k].copy_(b[k])
        graph.replay()
    res, flags = ev.result(return_flags=True)
    assert flags["tp"].numel() == sum(live) and exp["tp"].any()
    for k in ("best_iou", "best_gt", "tp"):
        assert torch.equal(flags[k], exp[k])
    assert res == exp_res


def test_add_takes_the_padded_nms_output(device):
    """nms_device(padded=True) -> add(n=n_out): the block as it lies (int64 labels, rows behind n_out undefined), no read in between"""
    from cnrma_amd import postprocess as PP
    g, d = one_scene(45, 300, 12, cols=6, n_classes=3)
    rng = np.random.default_rng(45)
    scores = torch.from_numpy(np.where(np.arange(3) == d["labels"][:, None], d["scores"][:, None], 0.0).astype(np.float32)).to(device)
    scores += torch.from_numpy(rng.uniform(0, 0.2, (300, 3)).astype(np.float32)).to(device)
    boxes = torch.from_numpy(d["boxes"]).to(device)
    gt_boxes, gt_labels = torch.from_numpy(g["boxes"]).to(device), torch.from_numpy(g["labels"]).to(device)
    ev, bufs = evaluator_for([g], [d], (0.25, 0.5), 3, device, det_capacity=900), PP.nms_device_buffers(300, 3, 6, device)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        b, s, l, n_out = PP.nms_device(boxes, scores, score_thr=0.05, iou_thr=0.5, padded=True, out=bufs)
        ev.add(b, s, l, gt_boxes, gt_labels, n=n_out)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    k = int(n_out.item())
    assert 12 < k < 900
    kept = dict(boxes=b[:k].cpu().numpy(), scores=s[:k].cpu().numpy(), labels=l[:k].cpu().numpy())
    ref = host_reference([g], [kept], (0.25, 0.5), 3, device)
    res, flags = ev.result(return_flags=True)
    assert_same_flags(flags, ref)
    assert_same_dict(res, ref["result"])
    assert ref["tp"].any()


def test_overflow_raises_and_reset_starts_afresh(device):
    from cnrma_amd._lib import CnrmaError
    (g0, d0), (g1, d1) = one_scene(50, 33, 6), one_scene(51, 20, 4)
    keep = []
    ev = guard_state(evaluator_for([g0], [d0], (0.25, 0.5), 2, device, det_capacity=32, gt_capacity=6, scene_capacity=1), keep)
    ev.add(d0["boxes"], d0["scores"], d0["labels"], g0["boxes"], g0["labels"])          # 33 rows into 32
    with pytest.raises(CnrmaError, match="det_capacity=32"):
        ev.result()
    ev.add(d1["boxes"], d1["scores"], d1["labels"], g1["boxes"], g1["labels"])          # a second scene, more boxes: nothing fits
    with pytest.raises(CnrmaError, match="capacity"):
        ev.result()
    torch.cuda.synchronize()
    assert guards_intact(keep)
    for cap, name in ((dict(gt_capacity=5), "gt_capacity=5"), (dict(scene_capacity=1), "scene_capacity=1")):
        small = guard_state(evaluator_for([g0, g1], [d0, d1], (0.25, 0.5), 2, device, **cap), keep)
        add_all(small, [g0, g1], [d0, d1])
        with pytest.raises(CnrmaError, match=name):
            small.result()
    torch.cuda.synchronize()
    assert guards_intact(keep)
    ev.reset()
    ev.add(d1["boxes"], d1["scores"], d1["labels"], g1["boxes"], g1["labels"])
    res, flags = ev.result(return_flags=True)
    exp_res, exp = add_all(evaluator_for([g1], [d1], (0.25, 0.5), 2, device), [g1], [d1]).result(return_flags=True)
    assert res == exp_res and torch.equal(flags["tp"], exp["tp"]) and torch.equal(flags["best_gt"], exp["best_gt"])
    assert guards_intact(keep)


def test_evaluator_without_detections_or_scenes(device):
    from cnrma_amd.evaluate import DetectionEvaluator
    from cnrma_amd import postprocess as PP
    assert DetectionEvaluator(3, device=device).result() == PP.indoor_eval([], [], n_classes=3)
    g, _ = one_scene(60, 4, 5)
    none = dict(boxes=np.zeros((0, 7), np.float32), scores=np.zeros(0, np.float32), labels=np.zeros(0, np.int64))
    assert PP.indoor_eval_device([g], [none], n_classes=2, device=device) == PP.indoor_eval([g], [none], n_classes=2, device=device)


# ---- argument rules ------------------------------------------------------------------------------------------------------------------
def test_refused_calls_leave_the_outputs_alone(device):
    from cnrma_amd import _lib
    lib = _lib.load_eval()
    f32 = lambda n, v=0.5: torch.full((n,), v, dtype=torch.float32, device=device)
    i32 = lambda n, v=0: torch.full((n,), v, dtype=torch.int32, device=device)
    outs = dict(best_iou=f32(3, -5.0), best_gt=i32(3, GUARD), flags=torch.full((3,), 77, dtype=torch.uint8, device=device),
                table=torch.full((2 * 3 * 4,), -5.0, dtype=torch.float64, device=device),
                workspace=torch.full((4096,), 77, dtype=torch.uint8, device=device))
    before = {k: v.clone() for k, v in outs.items()}
    p = _lib.ptr
    args = dict(det_boxes=p(f32(21)), det_labels=p(i32(3)), det_scene=p(i32(3)), n_det=3, gt_boxes=p(f32(14)), gt_labels=p(i32(2)),
                n_gt=2, scene_gt=p(i32(2)), n_scenes=1, rotated=0, order=p(torch.arange(3, device=device)),
                thresholds=p(f32(2, 0.25)), T=2, n_classes=3, workspace=p(outs["workspace"]), workspace_bytes=4096,
                best_iou=p(outs["best_iou"]), best_gt=p(outs["best_gt"]), flags=p(outs["flags"]), table=p(outs["table"]),
                stream=_lib.stream())
    for bad in (dict(n_det=-1), dict(n_gt=-1), dict(T=0), dict(T=9), dict(n_classes=0), dict(table=None), dict(det_boxes=None),
                dict(order=None), dict(workspace_bytes=16), dict(thresholds=None)):
        assert lib.cnrma_eval_result_f32(*dict(args, **bad).values()) == -22, bad
    counters = i32(4, 7)
    state = dict(boxes=f32(12), box_cols=6, scores=f32(2), labels=i32(2), label_bytes=4, n_rows=2, n_live=None, gt_boxes=f32(6),
                 gt_cols=6, gt_labels=i32(1), gt_label_bytes=4, n_gt=1, det_boxes=f32(70, -5.0), det_scores=f32(10, -5.0),
                 det_labels=i32(10, GUARD), det_scene=i32(10, GUARD), det_cap=10, st_gt_boxes=f32(70, -5.0),
                 st_gt_labels=i32(10, GUARD), gt_cap=10, scene_gt=i32(8, GUARD), scene_cap=4, counters=counters, stream=_lib.stream())
    raw = lambda d: [p(v) if torch.is_tensor(v) else v for v in d.values()]
    for bad in (dict(n_rows=-1), dict(n_gt=-1), dict(box_cols=5), dict(label_bytes=3), dict(det_cap=-1), dict(counters=None),
                dict(boxes=None)):
        assert lib.cnrma_eval_append_f32(*raw(dict(state, **bad))) == -22, bad
    torch.cuda.synchronize()
    assert all(torch.equal(outs[k], before[k]) for k in outs)
    assert counters.tolist() == [7] * 4 and bool((state["det_labels"] == GUARD).all()) and bool((state["det_boxes"] == -5).all())
    assert bool((state["scene_gt"] == GUARD).all()) and bool((state["st_gt_boxes"] == -5).all())


# ---- end to end ------------------------------------------------------------------------------------------------------------------------
def test_cli_device_equals_host(tmp_path, capsys, device):
    cats = [3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 14, 16, 24, 28, 33, 34, 36, 39]
    data, results = tmp_path / "data" / "scannet_instance_data", tmp_path / "results"
    data.mkdir(parents=True)
    for k, name in enumerate(("scene0000_00", "scene0001_00")):
        g, d = one_scene(70 + k, 40, 8, cols=6, n_classes=4)
        (results / name).mkdir(parents=True)
        np.savez(results / name / (name + "_atlas_bbox.npz"), boxes=d["boxes"], scores=d["scores"], labels=d["labels"])
        np.save(data / (name + "_aligned_bbox.npy"), np.concatenate((g["boxes"], np.array(cats)[g["labels"]][:, None]), axis=1))
    printed = {}
    for evaluator in ("host", "device"):
        argv = ["evaluate_bbox.py", "--data_path", str(tmp_path / "data"), "--result_path", str(results), "--evaluator", evaluator]
        old, sys.argv = sys.argv, argv
        try:
            runpy.run_path(os.path.join(ROOT, "post_process", "evaluate_bbox.py"), run_name="__main__")
        finally:
            sys.argv = old
        printed[evaluator] = ast.literal_eval(capsys.readouterr().out.strip().splitlines()[-1])
    assert sorted(printed["host"]) == ["mAP_0.25", "mAP_0.50", "mAR_0.25", "mAR_0.50"] and printed["host"]["mAP_0.25"] > 0
    assert_same_dict(printed["device"], printed["host"])
