"""Host-side tests of the device mAP evaluation: the C surface of libcnrma_eval_hip.so (include/cnrma_eval.h), its argument checks
(answered before any launch, so without a device), the float64 oracle tests/eval_oracle.py against hand-computed cases, and the
seeded data set's named scenes."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import eval_oracle as EO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, I, Z = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t
EVAL_TABLE = {
    "cnrma_eval_abi_version": (I, []),
    "cnrma_eval_reset": (I, [P, P]),
    "cnrma_eval_append_f32": (I, [P, I, P, P, I, I, P, P, I, P, I, I, P, P, P, P, I, P, P, I, P, I, P, P]),
    "cnrma_eval_result_workspace_bytes": (Z, [I, I, I]),
    "cnrma_eval_result_f32": (I, [P, P, P, I, P, P, I, P, I, I, P, P, I, I, P, Z, P, P, P, P, P]),
}


def eval_lib():
    from cnrma_amd import _lib
    if not os.path.exists(_lib.EVAL_LIB_PATH):                                   # fresh checkout: hipcc cross-compiles without a GPU
        subprocess.run(["make", "-C", os.path.dirname(_lib.EVAL_LIB_PATH), "-j8", "libcnrma_eval_hip.so"], check=True)
    return _lib.load_eval()


def test_header_is_read_without_experiments():
    from cnrma_amd import _lib
    with open(_lib.EVAL_HEADER_PATH) as f:
        table, exp, constants = _lib._read_header(f.read())
    assert exp == {} and table == EVAL_TABLE and list(table) == list(EVAL_TABLE)
    assert _lib.EVAL_SIGNATURES == EVAL_TABLE
    assert constants == {"CNRMA_EVAL_EINVAL": -22, "CNRMA_EVAL_ABI_VERSION": 1} and _lib.EVAL_ABI_VERSION == 1
    assert len(_lib.SIGNATURES) == 128 and _lib.ABI_VERSION == 7                 # the product surface is as it was
    assert not any(name.startswith("cnrma_eval_") for name in list(_lib.SIGNATURES) + list(_lib.EXPERIMENT_SIGNATURES))


def test_library_exports_exactly_the_header():
    from cnrma_amd import _lib
    lib = eval_lib()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.EVAL_LIB_PATH], check=True, capture_output=True, text=True).stdout
    names = {l.split()[-1] for l in out.splitlines() if l.split()[-1].startswith("cnrma_")}
    assert names == set(EVAL_TABLE)
    assert lib.cnrma_eval_abi_version() == 1
    if os.path.exists(_lib.LIB_PATH):                                            # the product library holds none of it
        out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
        assert not [l for l in out.splitlines() if "cnrma_eval_" in l]
    makefile = open(os.path.join(ROOT, "cn-rma_amd", "csrc", "Makefile")).read()
    assert "eval.o: eval.hip box_geom.h" in makefile and "nms.o: nms.hip box_geom.h" in makefile


def test_workspace_query():
    lib = eval_lib()
    q = lib.cnrma_eval_result_workspace_bytes
    assert q(0, 0, 1) > 0 and q(1000, 100, 2) >= 2 * 100 * 4 + 1000 and q(1000, 100, 2) % 16 == 0
    assert q(1000, 100, 8) - q(1000, 100, 2) == 6 * 100 * 4
    for bad in ((-1, 0, 1), (0, -1, 1), (0, 0, 0), (0, 0, 9)):
        assert q(*bad) == 0


RESULT_ARGS = dict(det_boxes=64, det_labels=64, det_scene=64, n_det=3, gt_boxes=64, gt_labels=64, n_gt=2, scene_gt=64, n_scenes=1,
                   rotated=0, order=64, thresholds=64, T=2, n_classes=3, workspace=64, workspace_bytes=1 << 20, best_iou=64,
                   best_gt=64, flags=64, table=64, stream=None)
RESULT_BAD = [dict(n_det=-1), dict(n_gt=-1), dict(n_scenes=-1), dict(T=0), dict(T=9), dict(n_classes=0), dict(n_classes=-2),
              dict(workspace_bytes=8), dict(workspace=None), dict(workspace=72), dict(table=None), dict(thresholds=None),
              dict(det_boxes=None), dict(det_labels=None), dict(det_scene=None), dict(order=None), dict(best_iou=None),
              dict(best_gt=None), dict(flags=None), dict(gt_boxes=None), dict(gt_labels=None), dict(scene_gt=None)]
APPEND_ARGS = dict(boxes=64, box_cols=6, scores=64, labels=64, label_bytes=8, n_rows=4, n_live=None, gt_boxes=64, gt_cols=6,
                   gt_labels=64, gt_label_bytes=8, n_gt=2, st_det_boxes=64, st_det_scores=64, st_det_labels=64, st_det_scene=64,
                   det_cap=16, st_gt_boxes=64, st_gt_labels=64, gt_cap=16, st_scene_gt=64, scene_cap=4, counters=64, stream=None)
APPEND_BAD = [dict(n_rows=-1), dict(n_gt=-1), dict(det_cap=-1), dict(gt_cap=-1), dict(scene_cap=-1), dict(box_cols=5),
              dict(box_cols=8), dict(gt_cols=3), dict(label_bytes=2), dict(gt_label_bytes=0), dict(counters=None),
              dict(boxes=None), dict(scores=None), dict(labels=None), dict(gt_boxes=None), dict(gt_labels=None),
              dict(st_det_boxes=None), dict(st_det_scores=None), dict(st_det_labels=None), dict(st_det_scene=None),
              dict(st_gt_boxes=None), dict(st_gt_labels=None), dict(st_scene_gt=None)]


@pytest.mark.parametrize("bad", RESULT_BAD, ids=lambda b: "-".join(f"{k}={v}" for k, v in b.items()))
def test_result_refuses_before_any_launch(bad):
    """the pointers are not device memory: a call that got past its checks would fault, not return"""
    assert eval_lib().cnrma_eval_result_f32(*dict(RESULT_ARGS, **bad).values()) == -22


@pytest.mark.parametrize("bad", APPEND_BAD, ids=lambda b: "-".join(f"{k}={v}" for k, v in b.items()))
def test_append_refuses_before_any_launch(bad):
    assert eval_lib().cnrma_eval_append_f32(*dict(APPEND_ARGS, **bad).values()) == -22


def test_reset_refuses_a_null_pointer():
    assert eval_lib().cnrma_eval_reset(None, None) == -22


def test_evaluator_arguments_raise_before_the_device_is_needed():
    from cnrma_amd.evaluate import DetectionEvaluator
    for kw in (dict(n_classes=0), dict(n_classes=3, iou_thrs=()), dict(n_classes=3, iou_thrs=(0.1,) * 9),
               dict(n_classes=3, iou_thrs=(1.0,)), dict(n_classes=3, iou_thrs=(-0.1,)), dict(n_classes=3, det_capacity=0),
               dict(n_classes=3, gt_capacity=0), dict(n_classes=3, scene_capacity=0)):
        with pytest.raises(ValueError):
            DetectionEvaluator(**kw)


def test_mixed_column_counts_are_a_value_error():
    from cnrma_amd.evaluate import indoor_eval_device
    six, seven = np.ones((2, 6), np.float32), np.ones((2, 7), np.float32)
    lab = np.zeros(2, np.int64)
    det = lambda b: dict(boxes=b, scores=np.ones(2, np.float32), labels=lab)
    with pytest.raises(ValueError):
        indoor_eval_device([dict(boxes=six, labels=lab)] * 2, [det(six), det(seven)])
    with pytest.raises(ValueError):
        indoor_eval_device([dict(boxes=six, labels=lab), dict(boxes=seven, labels=lab)], [det(six), det(six)])


# ---- the oracle against hand-computed cases -----------------------------------------------------------------------------------------
def test_oracle_ap_of_tp_fp_tp():
    ap, rec = EO.average_precision([True, False, True], 2)
    assert ap == pytest.approx(0.5 * 1 + 0.5 * (2 / 3), abs=1e-15) and rec == 1.0
    assert EO.average_precision([], 4) == (0.0, 0.0)
    assert EO.average_precision([False, False], 1) == (0.0, 0.0)
    ap, rec = EO.average_precision([False, True], 4)                               # a quarter of the recall at precision 1/2
    assert ap == pytest.approx(0.125, abs=1e-15) and rec == 0.25


def cube(x):
    return [x, 0.0, 0.0, 1.0, 1.0, 1.0]


def test_oracle_perfect_detections_have_ap_one():
    gts, _, n_classes = EO.make_dataset(0, 7, 7, duplicates=False)
    dts = [dict(boxes=g["boxes"], scores=EO.quantised_scores(np.random.default_rng(1), len(g["labels"])), labels=g["labels"])
           for g in gts]
    res, scenes = EO.evaluate(gts, dts, (0.25, 0.5), n_classes)
    for thr in ("0.25", "0.50"):
        assert res["mAP_" + thr] == pytest.approx(1.0, abs=1e-12) and res["mAR_" + thr] == 1.0
        assert len(res["AP_" + thr]) == n_classes - 1                              # the class without ground truth is left out
    assert all(m["tp"].all() for m in scenes)


def test_oracle_claims_are_per_threshold():
    """one box; the higher-scored detection overlaps it by 1/3, the other by 9/11: the first takes the box at 0.25 and does not
    take it at 0.5"""
    gt = [dict(boxes=np.array([cube(0.0)]), labels=np.array([0]))]
    dt = [dict(boxes=np.array([cube(0.5), cube(0.1)]), scores=np.array([0.9, 0.8]), labels=np.array([0, 0]))]
    res, (m,) = EO.evaluate(gt, dt, (0.25, 0.5), 1)
    np.testing.assert_allclose(m["best_iou"], [1 / 3, 0.9 / 1.1], rtol=1e-12)
    assert m["tp"].tolist() == [[True, False], [False, True]]
    assert res["AP_0.25"] == [1.0] and res["AP_0.50"] == [0.5] and res["mAR_0.25"] == res["mAR_0.50"] == 1.0


def test_oracle_second_identical_detection_is_a_false_positive():
    """two identical boxes, two identical detections: the argmax names the first box both times"""
    gt = [dict(boxes=np.array([cube(0.0), cube(0.0)]), labels=np.array([0, 0]))]
    dt = [dict(boxes=np.array([cube(0.0), cube(0.0)]), scores=np.array([0.5, 0.5]), labels=np.array([0, 0]))]
    res, (m,) = EO.evaluate(gt, dt, (0.25,), 1)
    assert m["best_gt"].tolist() == [0, 0] and m["tp"][:, 0].tolist() == [True, False]
    assert res["AP_0.25"] == [0.5] and res["mAR_0.25"] == 0.5


@pytest.mark.parametrize("regular", [1, 3])
def test_data_set_holds_the_named_scenes(regular):
    gts, dts, n_classes = EO.make_dataset(0, 6, 7, regular=regular)
    assert len(gts) == len(dts) == 12 and n_classes == regular + 2
    n = lambda a: len(a["labels"])
    assert n(gts[2]) and not n(dts[2]) and not n(gts[4]) and n(dts[4]) and not n(gts[6]) and not n(dts[6])
    assert (dts[8]["labels"] == 0).any() and not (gts[8]["labels"] == 0).any() and any((g["labels"] == 0).any() for g in gts)
    gl, dl = np.concatenate([g["labels"] for g in gts]), np.concatenate([d["labels"] for d in dts])
    assert (gl == regular).any() and not (dl == regular).any()                     # ground truth and no detections
    assert (dl == regular + 1).any() and not (gl == regular + 1).any()             # no ground truth anywhere
    g, d = gts[10], dts[10]
    assert (g["boxes"][0] == g["boxes"][1]).all() and g["labels"][:2].tolist() == [0, 0]
    twins = [(i, j) for i in range(n(d)) for j in range(i) if (d["boxes"][i] == d["boxes"][j]).all()]
    assert len(twins) == 1 and d["labels"][list(twins[0])].tolist() == [0, 0]
    assert gts[0]["boxes"].shape[1] == 7 and dts[0]["boxes"].shape[1] == 6
    scores = np.concatenate([d["scores"] for d in dts])
    assert scores.dtype == np.float32 and set(np.unique(scores)) <= {0.25 + 0.125 * k for k in range(6)}
    assert any(len(np.unique(d["scores"])) < n(d) for d in dts)                    # ties within a scene (and so across scenes)
