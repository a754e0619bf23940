"""Per-class 3D NMS on the device (postprocess.nms_device / cnrma_nms_classes_f32: rank, mask, scan, gather) against the host
path it replaces (postprocess.nms: one class at a time, greedy scan in Python) and the float64 oracle; inside a captured graph,
at the end of a StaticScene, and through the plugin's writer thread.  Every comparison with postprocess.nms is torch.equal: the
suppression test is the same device function, the candidate order the same stable sort."""
import ctypes
import importlib.util
import os
import runpy
import types

import numpy as np
import pytest
import torch

from oracle import post_oracle as PO

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _boxes(rng, n, yaw=True):
    """a dense cloud in a 4 m room (tests/test_post_gpu.py): keeps and suppressions both occur"""
    b = np.zeros((n, 7), dtype=np.float32)
    b[:, :3] = rng.rand(n, 3) * 4
    b[:, 3:6] = 0.3 + rng.rand(n, 3) * 1.2
    if yaw:
        b[:, 6] = rng.uniform(-3.2, 3.2, n)
    return b


def _same(got, exp):
    assert len(got) == len(exp) == 3
    for g, e, what in zip(got, exp, ("boxes", "scores", "labels")):
        assert g.dtype == e.dtype and g.shape == e.shape, (what, g.dtype, e.dtype, tuple(g.shape), tuple(e.shape))
        assert torch.equal(g, e), what


def _dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


# ---------------------------------------------------------------------------------------------------------------------
# equality with the host path
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 4095, 4096])
@pytest.mark.parametrize("n_cls", [1, 18])
@pytest.mark.parametrize("cols", [7, 6], ids=["rotated", "axis"])
def test_equals_the_host_path(device, cols, n_cls, n):
    """row counts on both sides of the 64-bit word and of the 4096-row limit; scores = u^3 (a fifth below the threshold).
    The boxes cover 0.8 m^2 of the 16 m^2 floor on average: thousands of them pile up dozens deep and suppress at IoU > 0.5,
    a few dozen only touch their neighbours -- there the threshold is 0.1, so that every case with more than one box has both
    kept and suppressed boxes"""
    from cnrma_amd import postprocess as PP
    rng = np.random.RandomState(1000 * cols + 10 * n_cls + n % 7)
    b = _dev(_boxes(rng, n, cols == 7)[:, :cols], device)
    s = _dev((rng.rand(n, n_cls) ** 3).astype(np.float32), device)
    iou_thr = 0.5 if n > 1000 else 0.1
    exp = PP.nms(b, s, 0.01, iou_thr)
    got = PP.nms_device(b, s, 0.01, iou_thr)
    _same(got, exp)
    candidates = int((s > 0.01).sum())
    assert len(got[0]) <= candidates
    if n >= 63:                                             # both outcomes occur: boxes are kept, boxes are suppressed
        assert 0 < len(got[0]) < candidates, (len(got[0]), candidates)
    else:
        assert len(got[0]) == candidates                    # a single row: kept in every class it is a candidate of


@pytest.mark.parametrize("yaw", [False, True])
def test_against_the_fp64_oracle(device, yaw):
    """the inputs of tests/test_post_gpu.py::test_nms_vs_oracle, where the mask kernel is known to agree with the oracle"""
    from cnrma_amd import postprocess as PP
    rng = np.random.RandomState(2)
    b = _boxes(rng, 300, yaw)
    s = rng.rand(300).astype(np.float32)
    exp = np.asarray(PO.nms(b, s, 0.3), dtype=np.int64)
    assert 10 < len(exp) < 300
    bb = b if yaw else b[:, :6]
    boxes, scores, labels = PP.nms_device(_dev(bb, device), _dev(s[:, None], device), score_thr=-1.0, iou_thr=0.3)
    assert np.array_equal(boxes.cpu().numpy(), bb[exp]) and np.array_equal(scores.cpu().numpy(), s[exp])
    assert labels.dtype == torch.long and not labels.any()


# ---------------------------------------------------------------------------------------------------------------------
# edge cases
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cols", [7, 6])
def test_no_candidate_in_any_class(device, cols):
    from cnrma_amd import postprocess as PP
    rng = np.random.RandomState(3)
    b = _dev(_boxes(rng, 130)[:, :cols], device)
    s = _dev((rng.rand(130, 5) * 0.01).astype(np.float32), device)          # all <= the threshold
    s[7, 2] = float("nan")                                                   # NaN never passes
    got = PP.nms_device(b, s, 0.01, 0.5)
    _same(got, PP.nms(b, s, 0.01, 0.5))
    assert tuple(got[0].shape) == (0, cols) and got[0].dtype == torch.float32
    assert tuple(got[1].shape) == (0,) and got[1].dtype == torch.float32
    assert tuple(got[2].shape) == (0,) and got[2].dtype == torch.long
    assert int(PP.nms_device(b, s, 0.01, 0.5, padded=True)[3].cpu()) == 0
    empty = PP.nms_device(b[:0], s[:0], 0.01, 0.5)                           # no row at all
    assert tuple(empty[0].shape) == (0, cols) and tuple(empty[1].shape) == (0,) and empty[2].dtype == torch.long


@pytest.mark.parametrize("levels", [1, 2, 5])
def test_equal_scores_keep_the_stable_order(device, levels):
    """whole groups of equal scores (one value for everything at levels = 1): ties go by the lower row, as in torch's stable sort"""
    from cnrma_amd import postprocess as PP
    rng = np.random.RandomState(4 + levels)
    n = 700
    b = _dev(_boxes(rng, n), device)
    s = _dev((0.25 + 0.125 * rng.randint(0, levels, (n, 3))).astype(np.float32), device)
    s[25::50, 1] = -0.0                                                       # signed zeros tie as well (below the threshold here)
    got = PP.nms_device(b, s, 0.01, 0.5)
    _same(got, PP.nms(b, s, 0.01, 0.5))
    assert 3 < len(got[0]) < 3 * n
    if levels == 1:                                                          # every box ties: row 0 comes first in every class
        for c in range(3):
            assert torch.equal(got[0][got[2] == c][0], b[0])
    zeros = _dev(np.where(rng.rand(n, 2) < 0.5, 0.0, -0.0).astype(np.float32), device)     # +0.0 and -0.0 are ONE score
    _same(PP.nms_device(b, zeros, -1.0, 0.5), PP.nms(b, zeros, -1.0, 0.5))


@pytest.mark.parametrize("cols", [7, 6])
def test_identical_boxes_keep_one_per_class(device, cols):
    from cnrma_amd import postprocess as PP
    rng = np.random.RandomState(5)
    n, n_cls = 200, 4
    one = np.array([1.0, 2.0, 0.5, 0.8, 0.6, 1.0, 0.3], dtype=np.float32)[:cols]
    b = _dev(np.tile(one, (n, 1)), device)
    s = _dev((0.1 + 0.8 * rng.rand(n, n_cls)).astype(np.float32), device)
    boxes, scores, labels = got = PP.nms_device(b, s, 0.01, 0.5)
    _same(got, PP.nms(b, s, 0.01, 0.5))
    assert labels.tolist() == list(range(n_cls)) and torch.equal(scores, s.max(0).values)


@pytest.mark.parametrize("cols", [7, 6])
def test_a_suppressed_box_suppresses_nothing(device, cols):
    """A suppresses B, B overlaps C, A does not overlap C: greedy NMS keeps C ("overlaps anything" would drop it)"""
    from cnrma_amd import postprocess as PP
    b = np.zeros((3, 7), dtype=np.float32)
    b[:, 3:6] = 1.0
    b[:, 0] = (0.0, 0.3, 0.6)                                # IoU(A, B) = IoU(B, C) = 0.7 / 1.3, IoU(A, C) = 0.4 / 1.6
    s = np.array([[0.9], [0.8], [0.7]], dtype=np.float32)
    b, s = _dev(b[:, :cols], device), _dev(s, device)
    boxes, scores, labels = got = PP.nms_device(b, s, 0.01, 0.5)
    _same(got, PP.nms(b, s, 0.01, 0.5))
    assert torch.equal(boxes, b[[0, 2]]) and scores.tolist() == [pytest.approx(0.9), pytest.approx(0.7)]
    # the same chain across a word boundary: 62 far-away boxes in front, so that B and C sit in ranks 63 and 64
    far = np.zeros((62, 7), dtype=np.float32)
    far[:, 3:6] = 1.0
    far[:, 1] = 10.0 + 2.0 * np.arange(62)
    b2 = torch.cat((_dev(far[:, :cols], device), b))
    s2 = torch.cat((torch.ones(62, 1, device=device), s))
    got2 = PP.nms_device(b2, s2, 0.01, 0.5)
    _same(got2, PP.nms(b2, s2, 0.01, 0.5))
    assert len(got2[0]) == 64 and torch.equal(got2[0][-2:], b[[0, 2]])


@pytest.mark.parametrize("cols", [7, 6])
def test_both_thresholds_are_strict(device, cols):
    """score == score_thr is no candidate; IoU == iou_thr does not suppress: two unit squares half a side apart overlap in 1/2 of
    a union of 3/2, and 0.5f / 1.5f is the float32 nearest to 1/3 -- the value the threshold 1/3 is passed as"""
    from cnrma_amd import postprocess as PP
    b = np.zeros((3, 7), dtype=np.float32)
    b[:, 3:6] = 1.0
    b[1, 0] = 0.5
    b[2, 1] = 5.0
    b = _dev(b[:, :cols], device)
    above = float(np.nextafter(np.float32(0.25), np.float32(1)))
    s = _dev(np.array([[0.75, 0.25], [0.5, above], [0.25, 0.25]], dtype=np.float32), device)
    third = 1.0 / 3.0
    boxes, scores, labels = got = PP.nms_device(b, s, 0.25, third)
    _same(got, PP.nms(b, s, 0.25, third))
    assert labels.tolist() == [0, 0, 1] and torch.equal(boxes, b[[0, 1, 1]])        # row 2 (score == thr) is in no class
    below = float(np.nextafter(np.float32(third), np.float32(0)))
    got = PP.nms_device(b, s, 0.25, below)
    _same(got, PP.nms(b, s, 0.25, below))
    assert got[2].tolist() == [0, 1] and torch.equal(got[0], b[[0, 1]])


@pytest.mark.parametrize("cols", [7, 6])
def test_a_box_without_area_suppresses_nothing(device, cols):
    from cnrma_amd import postprocess as PP
    b = np.zeros((4, 7), dtype=np.float32)
    b[:, 3:6] = 1.0
    b[0, 3] = 0.0                                            # the best box has no width: it sits inside the others
    b[2, 4] = 0.0                                            # so does a lesser one
    s = np.array([[0.9], [0.8], [0.7], [0.6]], dtype=np.float32)
    b, s = _dev(b[:, :cols], device), _dev(s, device)
    boxes, scores, labels = got = PP.nms_device(b, s, 0.01, 0.5)
    _same(got, PP.nms(b, s, 0.01, 0.5))
    assert torch.equal(boxes, b[[0, 1, 2]])                  # only the full box 3 goes, suppressed by its twin 1


# ---------------------------------------------------------------------------------------------------------------------
# the padded block of the static trace
# ---------------------------------------------------------------------------------------------------------------------
SIZES, VALID = [100, 64, 37, 130], [60, 0, 37, 129]          # one segment empty, one full


def _padded_case(device, cols, seed, n_cls=6):
    rng = np.random.RandomState(seed)
    n = sum(SIZES)
    b = _boxes(rng, n, cols == 7)[:, :cols]
    s = (rng.rand(n, n_cls) ** 2).astype(np.float32)
    live, r0 = [], 0
    for k, v in zip(SIZES, VALID):
        live += list(range(r0, r0 + v))
        dead = np.arange(r0 + v, r0 + k)
        b[dead[::2]], s[dead[::2]] = np.nan, np.nan          # dead rows: NaN ...
        s[dead[1::2]] = 3.0e38                               # ... and scores that would win every class
        r0 += k
    return _dev(b, device), _dev(s, device), torch.tensor(live, device=device)


@pytest.mark.parametrize("cols", [7, 6])
def test_padded_segments_equal_the_compacted_block(device, cols):
    from cnrma_amd import postprocess as PP
    b, s, live = _padded_case(device, cols, 6)
    valid = torch.tensor(VALID, dtype=torch.int32, device=device)
    exp = PP.nms(b[live], s[live], 0.01, 0.5)
    assert 0 < len(exp[0]) < int((s[live] > 0.01).sum())
    _same(PP.nms_device(b, s, 0.01, 0.5, valid=valid, sizes=SIZES), exp)
    boxes, scores, labels, n_out = PP.nms_device(b, s, 0.01, 0.5, valid=valid, sizes=SIZES, padded=True)
    k = int(n_out.cpu())
    assert n_out.dtype == torch.int32 and boxes.shape[0] >= k == len(exp[0])
    _same((boxes[:k], scores[:k], labels[:k]), exp)


def _raw_call(device, n_cap, n_cls=2, cols=7):
    from cnrma_amd import _lib
    lib = _lib.load()
    b = torch.zeros((n_cap, cols), device=device)
    s = torch.zeros((n_cap, n_cls), device=device)
    ws = torch.zeros(1 << 20, dtype=torch.uint8, device=device)
    ob, os_, ol = torch.zeros((8, cols), device=device), torch.zeros(8, device=device), torch.zeros(8, dtype=torch.long, device=device)
    n_out = torch.full((1,), -5, dtype=torch.int32, device=device)
    sizes = (ctypes.c_int32 * 1)(n_cap)
    rc = lib.cnrma_nms_classes_f32(b.data_ptr(), cols, s.data_ptr(), n_cap, n_cls, ctypes.addressof(sizes), 1, None, 0.01, 0.5,
                                   ws.data_ptr(), ws.numel(), ob.data_ptr(), os_.data_ptr(), ol.data_ptr(), 8, n_out.data_ptr(),
                                   _lib.stream())
    torch.cuda.synchronize()
    return rc, int(n_out.cpu())


def test_more_than_4096_rows_are_refused_by_the_kernel_and_served_by_the_host_path(device):
    from cnrma_amd import postprocess as PP
    assert _raw_call(device, 4097) == (-22, -5)              # CNRMA_EINVAL, nothing launched
    assert _raw_call(device, 64, cols=5)[0] == -22 and _raw_call(device, 64, n_cls=0)[0] == -22
    assert _raw_call(device, 64) == (0, 0)                   # the same call inside the limit (all scores 0: no candidate)
    rng = np.random.RandomState(7)
    b, s = _dev(_boxes(rng, 4097), device), _dev((rng.rand(4097, 2) ** 3).astype(np.float32), device)
    _same(PP.nms_device(b, s, 0.01, 0.5), PP.nms(b, s, 0.01, 0.5))
    with pytest.raises(Exception):
        PP.nms_device(b, s, 0.01, 0.5, padded=True)          # no quiet substitute for the capturable form


def test_output_overflow_reports_the_true_total(device):
    from cnrma_amd import postprocess as PP
    rng = np.random.RandomState(8)
    b, s = _dev(_boxes(rng, 500), device), _dev((rng.rand(500, 7) ** 3).astype(np.float32), device)
    exp = PP.nms(b, s, 0.01, 0.5)
    total = len(exp[0])
    cap = total // 2
    assert cap >= 7
    boxes, scores, labels, n_out = PP.nms_device(b, s, 0.01, 0.5, padded=True, out_cap=cap)
    assert boxes.shape[0] == cap and int(n_out.cpu()) == total
    _same((boxes, scores, labels), tuple(t[:cap] for t in exp))
    _same(PP.nms_device(b, s, 0.01, 0.5, out_cap=cap), tuple(t[:cap] for t in exp))


def test_capture_and_replay_on_new_inputs(device):
    """the padded form inside torch.cuda.graph on a side stream: a device->host read in there would abort the capture; every
    replay equals the eager result on the inputs copied into the static buffers"""
    from cnrma_amd import postprocess as PP
    cases = [_padded_case(device, 7, seed) for seed in (11, 12)]
    n, n_cls = cases[0][0].shape[0], cases[0][1].shape[1]
    sb, ss = torch.zeros_like(cases[0][0]), torch.zeros_like(cases[0][1])
    valid = torch.tensor(VALID, dtype=torch.int32, device=device)
    bufs = PP.nms_device_buffers(n, n_cls, 7, device)
    side = torch.cuda.Stream(device=device)
    side.wait_stream(torch.cuda.current_stream(device))
    with torch.cuda.stream(side):                            # once eagerly: the kernels' code is loaded before the capture
        PP.nms_device(sb, ss, 0.01, 0.5, valid=valid, sizes=SIZES, padded=True, out=bufs)
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        out = PP.nms_device(sb, ss, 0.01, 0.5, valid=valid, sizes=SIZES, padded=True, out=bufs)
    torch.cuda.synchronize()
    for b, s, live in cases + cases[:1]:
        sb.copy_(b)
        ss.copy_(s)
        graph.replay()
        torch.cuda.synchronize()
        k = int(out[3].cpu())
        got = tuple(t[:k].clone() for t in out[:3])
        _same(got, PP.nms_device(b, s, 0.01, 0.5, valid=valid, sizes=SIZES))
        _same(got, PP.nms(b[live], s[live], 0.01, 0.5))
        assert 0 < k < len(live) * n_cls


# ---------------------------------------------------------------------------------------------------------------------
# at the end of a scene graph
# ---------------------------------------------------------------------------------------------------------------------
def _model(C, dev, n_classes=18, n_reg=6):
    from projects.mvsdetection.models.fcaf3d_backbone import FCAF3DBackbone
    from projects.mvsdetection.models.fcaf3d_head import FCAF3DHead
    torch.manual_seed(0)
    backbone = FCAF3DBackbone(C, 34)
    head = FCAF3DHead(n_classes, (64, 128, 256, 512), 128, n_reg, 0.01, 2000, None, test_cfg=dict(nms_pre=100))
    backbone.init_weights()
    head.init_weights()
    return backbone.to(dev).eval(), head.to(dev).eval()


def _confident(head):
    """a freshly initialised head scores every class at 0.01 x centerness 0.5: nothing passes score_thr = 0.01 and the NMS would have
    nothing to do.  Three units on the classification bias lift the scores to about 0.17 x 0.5, so that most rows are
    candidates of every class and the dense rows of a level suppress one another"""
    with torch.no_grad():
        head.cls_conv.bias.add_(3.0)
    head._fused_head = None


def _scene(shape, seed, dev, boxes=0):
    from cnrma_amd import synth
    sc = synth.make_scene(shape, seed=seed, boxes=boxes)
    return sc, sc["features"][:, 0].to(dev), sc["projection"][:, 0], sc["tsdf"][0, 0].to(dev)


def test_static_scene_ends_with_the_final_detections(device):
    from cnrma_amd import pipeline
    from cnrma_amd import postprocess as PP
    sc, feat, proj, tsdf = _scene("tiny", 0, device)
    backbone, head = _model(feat.shape[1], device)
    _confident(head)
    cfg = pipeline.SceneConfig(sc["dims"], stride=sc["stride"], max_points=20000, sample_seed=1234)
    st = pipeline.StaticScene(cfg, backbone, head, device, nms=dict(score_thr=0.01, iou_thr=0.5))
    st.build(feat, proj, tsdf)
    assert st.graph is not None
    inputs = [(feat, proj, tsdf), _scene("tiny", 5, device)[1:], (feat, proj, tsdf)]
    for f, p, t in inputs:                                  # three replays, two different scenes
        out = st.run(f, p, t)
        torch.cuda.synchronize()
        assert out["nms_n"].dtype == torch.int32 and out["nms_labels"].dtype == torch.long
        got = pipeline.StaticScene.final_detections(out)
        exp = PP.nms(*pipeline.StaticScene.detections(out)[:2], score_thr=0.01, iou_thr=0.5)
        _same(got, exp)
        assert 0 < len(got[0]) < int((pipeline.StaticScene.detections(out)[1] > 0.01).sum())      # kept and suppressed boxes
    # off by default: the same graph as a slot built without the argument, node for node, and no new output
    plain = pipeline.StaticScene(cfg, backbone, head, device)
    plain.build(feat, proj, tsdf)
    off = pipeline.StaticScene(cfg, backbone, head, device, nms=None)
    off.build(feat, proj, tsdf)
    out = off.run(feat, proj, tsdf)
    torch.cuda.synchronize()
    assert not [k for k in out if k.startswith("nms_")]
    assert off.n_nodes == plain.n_nodes
    if plain.n_nodes is not None:
        # rank, mask, scan, gather; this plan has levels that keep all their rows, whose capacity (recorded size x margin) exceeds
        # nms_pre = 100: their segments are cut to 100 rows first (one copy of the boxes, one of the scores)
        assert max(out["sizes"]) > 100 and st.n_nodes == plain.n_nodes + 4 + 2
    with pytest.raises(Exception):
        pipeline.StaticScene.final_detections(out)           # a slot without the stage has no final detections


def test_static_net_ends_with_the_final_detections(device):
    """the sparse half alone (StaticNet) takes the same setting"""
    from cnrma_amd import pipeline
    from cnrma_amd import postprocess as PP
    from oracle import rma_oracle as O
    sc, feat, proj, tsdf = _scene("tiny", 0, device)
    backbone, head = _model(feat.shape[1], device)
    _confident(head)
    pts = O.aggregate_rma(sc["projection"][:, 0], sc["features"][:, 0], sc["tsdf"][0, 0], sc["dims"], 0.04, sc["origin"],
                          sc["stride"]).to(device)
    net = pipeline.StaticNet(backbone, head, 0.01, device, nms=dict(score_thr=0.01, iou_thr=0.5))
    net.build(pts[:, :3].contiguous(), pts[:, 3:].contiguous())
    out = net.run(pts[:, :3].contiguous(), pts[:, 3:].contiguous())
    torch.cuda.synchronize()
    got = pipeline.StaticNet.final_detections(out)
    _same(got, PP.nms(*pipeline.StaticScene.detections(out)[:2], score_thr=0.01, iou_thr=0.5))
    assert len(got[0]) > 0


# ---------------------------------------------------------------------------------------------------------------------
# through the plugin
# ---------------------------------------------------------------------------------------------------------------------
def _detector(tmp_path, dims, device, max_points, **kw):
    import projects.mvsdetection  # noqa: F401
    from projects.mvsdetection.registry import build_model
    cfg = runpy.run_path(os.path.join(ROOT, "projects", "configs", "mvsdetection", "ray_marching_scannet.py"))
    m = dict(cfg["model"])
    m.update(backbone2d=None, feature_2d=None, backbone_3d=None, tsdf_head=None)      # hot path only: features / TSDF come in
    m.update(save_path=str(tmp_path / "results"), voxel_dim_test=list(dims), voxel_dim_train=list(dims), max_points=max_points)
    m.update(kw)
    m["detection_backbone"] = dict(type="FCAF3DBackbone", in_channels=8, depth=34)
    model = build_model(m)
    torch.manual_seed(0)
    model.detection_backbone.init_weights()
    model.detection_head.init_weights()
    _confident(model.detection_head)
    return model.to(device).eval()


def _tiny_scenes(device, n):
    from cnrma_amd import synth
    out = []
    for i in range(n):
        sc = synth.make_scene("tiny", seed=i, boxes=i % 3)
        out.append(dict(features=[sc["features"][:, 0].to(device)], projection=[sc["projection"][:, 0].to(device)],
                        tsdf=sc["tsdf"].to(device), offset=[torch.tensor([0.25 * i, -0.5, 0.125 * (i % 2)], device=device)],
                        scene=[f"scene{i:04d}_00"]))
    return out


def test_plugin_writes_the_file_the_offline_step_would(device, tmp_path):
    """static_nms: {scene}_atlas_bbox.npz appears next to the raw file and holds what post_process/nms_bbox.py makes of that raw
    file -- which in turn is what the class-by-class host path makes of it"""
    from cnrma_amd import postprocess as PP
    from cnrma_amd import synth
    dims = synth.SHAPES["tiny"][4]
    model = _detector(tmp_path, dims, device, max_points=500000, static_nms=dict(score_thr=0.01, iou_thr=0.5))
    scenes = _tiny_scenes(device, 5)
    with torch.no_grad():
        for d in scenes:
            assert model(return_loss=False, **d) == [{}]
    model.flush()
    ctx = next(iter(model._static.values()))
    assert ctx["built"] and ctx["k"] == 5 - model.static_calibration and getattr(model, "static_fallbacks", 0) == 0
    spec = importlib.util.spec_from_file_location("nms_bbox_cli", os.path.join(ROOT, "post_process", "nms_bbox.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    cli.nms_bboxes(types.SimpleNamespace(result_path=str(tmp_path / "results"), postfix="_offline.npz"))
    for d in scenes:
        n = d["scene"][0]
        got = np.load(tmp_path / "results" / n / f"{n}_atlas_bbox.npz")
        off = np.load(tmp_path / "results" / n / f"{n}_offline.npz")
        raw = np.load(tmp_path / "results" / n / f"{n}_bbox_raw.npz")
        host = PP.nms(torch.tensor(raw["bboxes"]).to(device), torch.tensor(raw["scores"]).to(device))
        assert set(got.files) == set(off.files) == {"boxes", "scores", "labels"}
        for key, h in zip(("boxes", "scores", "labels"), host):
            assert got[key].dtype == off[key].dtype == h.cpu().numpy().dtype
            assert np.array_equal(got[key], off[key]) and np.array_equal(off[key], h.cpu().numpy()), (n, key)
        assert len(got["boxes"]) > 0
    # the default leaves the raw file alone
    plain = _detector(tmp_path / "plain", dims, device, max_points=500000)
    assert plain.static_nms is None
