"""Which C-ABI calls the host wrappers issue, as text: python scripts/launch_trace.py > LOG

Replaces `call` in cnrma_amd._lib, sparse, rma, cloud, mesh, fusion and postprocess with a recorder and prints one line per call:
the entry point and every argument, pointers reduced to NULL / ptr (the argument types come from _lib.SIGNATURES).  Two trees whose
logs are equal issue the same launches with the same scalar arguments in the same order.  Fixed-seed cases, each under a header line:

  train fp32 / bf16 [unfused]   forward + backward of a train-mode BasicBlock(32 -> 64, stride 2, downsample) and a Bottleneck(64, 16)
                                on ~300 voxels, in fp32 and under bf16 autocast, with FUSE_CONV_BN on and off
  aggregate all / sampled       eager rma.aggregate_points on the tiny synthetic scene, every row and a device-sampled half
  static scene                  StaticScene.build + one run on the tiny scene (what smoke() does)
  cloud, mesh                   eval_mesh on 1 000 random points a side; marching_cubes on the tiny TSDF
  static batch                  StaticBatch.build + one run of 2 tiny scenes under the static scene's calibrated plan
  head select                   the FCAF3D head's pruning and pre-NMS cut on the synthetic rows of tests/head_select_model.py, k = 64,
                                k-1, k, k+1 and 2k+3 rows, one scene and three scenes of which one is empty: _prune eager and static
                                (flags False and True, B = 1 and 3); get_bboxes, get_bboxes_fused, get_bboxes_static (flags True,
                                False, None), get_bboxes_static_multi

The selection code of the head is half torch ops, which the recorder does not see: the last two groups also print, indented and
interleaved with the C-ABI lines, every aten op that reaches the device (name, argument shapes and dtypes -> results).  Views and
bare allocations launch nothing and are left out.
"""
import ctypes
import os
import sys

import numpy as np
import torch
from torch.utils._python_dispatch import TorchDispatchMode
from torch.utils._pytree import tree_leaves

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from cnrma_amd import _lib, cloud, fusion, mesh, pipeline, postprocess, rma, synth  # noqa: E402
from cnrma_amd import nn as snn, plan as P, sparse as S  # noqa: E402

_call = _lib.call
_TABLE = dict(_lib.SIGNATURES, **_lib.EXPERIMENT_SIGNATURES)


def recorder(name, *args):
    types = _TABLE[name][1]
    assert len(types) == len(args), name
    shown = [("NULL" if not a else "ptr") if t is ctypes.c_void_p else repr(a) for t, a in zip(types, args)]
    print(name, *shown)
    return _call(name, *args)


class AtenOps(TorchDispatchMode):
    """prints every aten op with a device tensor among its arguments or results, except views and bare allocations"""
    QUIET = ("aten.empty.memory_format", "aten.empty_strided.default", "aten.empty_like.default")

    @staticmethod
    def show(a):
        if torch.is_tensor(a):
            return f"{str(a.dtype)[6:]}{list(a.shape)}"
        return str(a) if isinstance(a, (torch.dtype, torch.device)) else repr(a)

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        out = func(*args, **(kwargs or {}))
        ins, outs = tree_leaves((args, kwargs)), tree_leaves(out)
        if not func.is_view and str(func) not in self.QUIET and any(torch.is_tensor(t) and t.is_cuda for t in ins + outs):
            print("   ", func, *[self.show(a) for a in ins if a is not None], "->", *[self.show(o) for o in outs])
        return out


def block_case(dev, autocast, fused):
    rng = np.random.RandomState(5)
    c = np.unique(np.concatenate((np.zeros((340, 1), dtype=np.int64), rng.randint(-5, 5, size=(340, 3))), axis=1), axis=0)
    f = rng.randn(len(c), 32).astype(np.float32)
    torch.manual_seed(7)
    down = snn.FusedSequential(snn.MinkowskiConvolution(32, 64, kernel_size=1, stride=2, dimension=3), snn.MinkowskiBatchNorm(64))
    net = torch.nn.Sequential(snn.BasicBlock(32, 64, stride=2, downsample=down), snn.Bottleneck(64, 16)).to(dev).train()
    x = S.SparseTensor(torch.from_numpy(f).to(dev).requires_grad_(True), S.CoordSet(torch.from_numpy(c.astype(np.int32)).to(dev), 1))
    print(f"# train {'bf16' if autocast else 'fp32'}{'' if fused else ' unfused'}: {len(c)} voxels")
    S.FUSE_CONV_BN = fused
    try:
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
            y = net(x)
        y.F.backward(torch.ones_like(y.F))
    finally:
        S.FUSE_CONV_BN = True


K, TS, N_CLS = 64, 8, 18       # the cut / threshold, the rows' tensor stride and the classes of the head-select cases


def _static(flags, dev, fn):
    """fn() as a static trace under a hand-made plan with these flags"""
    plan = P.Plan()
    plan.flags = list(flags)
    plan.begin_static()
    with P.using(plan), torch.no_grad():
        out = fn()
        plan.status(dev)
    plan.end_static()
    return out


def _prune_inputs(counts, dev, static):
    import head_select_model as M
    from helpers import capacity_tensor
    lv = M.prune_level(counts, K, "plain", TS, seed=11)
    cap = (lambda n: n + 37) if static else (lambda n: None)
    return (capacity_tensor(lv["coords"], lv["feats"], TS, dev, cap=cap(len(lv["coords"])), n_batch=len(counts)),
            capacity_tensor(lv["score_coords"], lv["score"], 2 * TS, dev, cap=cap(len(lv["score"])), n_batch=len(counts)))


def _cut_inputs(layout, dev, static):
    """the five output lists of forward(..., fused=True) for four levels with these rows per scene"""
    import head_select_model as M
    from helpers import capacity_tensor, poison_rows
    lists = [[] for _ in range(5)]
    for li, counts in enumerate(layout):
        lv = M.cut_level(counts, K, "plain", N_CLS, seed=li)
        n = len(lv["scene"])
        pts, box = M.identity_rows(n, 6)
        coords = np.concatenate((lv["scene"][:, None], M.site(np.arange(n), TS)), axis=1)
        x = capacity_tensor(coords, lv["cen"], TS, dev, cap=n + 37 if static else None, n_batch=len(counts))
        x.cs.scene_major = True
        rest = [poison_rows(a, x.cs.n, dev) for a in (box, lv["cls"], pts)]
        for lst, t in zip(lists, [x.F] + rest + [x.cs]):
            lst.append([t])
    return lists


def head_select_cases(dev):
    from projects.mvsdetection.models.fcaf3d_head import FCAF3DHead
    head = FCAF3DHead(N_CLS, (8, 8, 8, 8), 8, 6, 0.01, K, None, test_cfg=dict(nms_pre=K)).eval()
    one = [(K - 1,), (K,), (K + 1,), (2 * K + 3,)]
    three = [(2 * K + 3, 0, K - 1), (K, K + 1, 0), (0, K - 1, K), (K + 1, 2 * K + 3, 0)]

    def case(title, fn, *inputs):
        print(f"# head select: {title}")
        with AtenOps(), torch.no_grad():
            fn(*inputs)

    for counts in one + three:
        case(f"_prune eager, rows per scene {counts}", head._prune, *_prune_inputs(counts, dev, False))
    for flag in (False, True):
        for counts in one + three:
            x, scores = _prune_inputs(counts, dev, True)
            case(f"_prune static, flag {flag}, rows per scene {counts}", lambda: _static([flag], dev, lambda: head._prune(x, scores)))
    cen, box, cls, pts, css = _cut_inputs(one, dev, False)
    case(f"get_bboxes, one scene, rows per level {one}", head.get_bboxes, cen, box, cls, pts, None, None)
    case(f"get_bboxes_fused, one scene, rows per level {one}", head.get_bboxes_fused, cen, box, cls, pts, css, 1)
    lists = _cut_inputs(three, dev, False)
    case(f"get_bboxes_fused, three scenes, rows per level and scene {three}", head.get_bboxes_fused, *lists, 3)
    lists = _cut_inputs(one, dev, True)
    for flag in (True, False, None):
        case(f"get_bboxes_static, flag {flag} on every level, rows per level {one}",
             lambda: _static([flag] * 4, dev, lambda: head.get_bboxes_static(*lists)))
    lists = _cut_inputs(three, dev, True)
    case(f"get_bboxes_static_multi, rows per level and scene {three}",
         lambda: _static([None] * 4, dev, lambda: head.get_bboxes_static_multi(*lists, 3)))


def main():
    dev = torch.device("cuda:0")
    for m in (_lib, S, rma, cloud, mesh, fusion, postprocess):
        m.call = recorder
    for fused in (True, False):
        for autocast in (False, True):
            block_case(dev, autocast, fused)

    sc = synth.make_scene("tiny", seed=0)
    feat, proj, tsdf = sc["features"][:, 0].to(dev), sc["projection"][:, 0], sc["tsdf"][0, 0].to(dev)
    torch.manual_seed(0)
    rma._SAMPLE_CALLS[0] = 0
    args = (rma.to_nhwc(feat), rma.projection_inverse(proj, sc["stride"]), tsdf, sc["dims"], 0.04, sc["origin"])
    print("# aggregate all")
    M = rma.aggregate_points(*args)[2]["M"]
    print(f"# aggregate sampled: {M // 2} of {M} rows")
    rma.aggregate_points(*args, max_points=M // 2, sampler="device")

    print("# static scene")
    from projects.mvsdetection.models.fcaf3d_backbone import FCAF3DBackbone
    from projects.mvsdetection.models.fcaf3d_head import FCAF3DHead
    torch.manual_seed(0)
    backbone = FCAF3DBackbone(feat.shape[1], 34).eval()
    head = FCAF3DHead(18, (64, 128, 256, 512), 128, 6, 0.01, 200000, None, test_cfg=dict(nms_pre=1000)).eval()
    head.init_weights()
    slot = pipeline.StaticScene(pipeline.SceneConfig(sc["dims"], stride=sc["stride"], max_points=None), backbone.to(dev),
                                head.to(dev), dev)
    slot.build(feat, proj, tsdf)
    slot.run(feat, proj, tsdf)["done"].synchronize()

    print("# cloud, mesh")
    rng = np.random.RandomState(3)
    cloud.eval_mesh(rng.rand(1000, 3).astype(np.float32), rng.rand(1000, 3).astype(np.float32))
    mesh.marching_cubes(tsdf, 0.04, sc["origin"])
    torch.cuda.synchronize()

    print("# static batch")
    scenes = [(feat, proj, tsdf), (feat, proj, tsdf)]
    batch = pipeline.StaticBatch(slot.cfg, slot.backbone, slot.head, dev, 2)
    with AtenOps():
        batch.build(scenes, slot.plan)
        batch.run(scenes)["done"].synchronize()
    head_select_cases(dev)
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
