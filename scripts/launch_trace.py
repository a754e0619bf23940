"""Which C-ABI calls the host wrappers issue, as text: python scripts/launch_trace.py > LOG

Replaces `call` in cnrma_amd._lib, sparse, rma, cloud, mesh, fusion and postprocess with a recorder and prints one line per call:
the entry point and every argument, pointers reduced to NULL / ptr (the argument types come from _lib.SIGNATURES).  Two trees whose
logs are equal issue the same launches with the same scalar arguments in the same order.  Fixed-seed cases, each under a header line:

  train fp32 / bf16 [unfused]   forward + backward of a train-mode BasicBlock(32 -> 64, stride 2, downsample) and a Bottleneck(64, 16)
                                on ~300 voxels, in fp32 and under bf16 autocast, with FUSE_CONV_BN on and off
  aggregate all / sampled       eager rma.aggregate_points on the tiny synthetic scene, every row and a device-sampled half
  static scene                  StaticScene.build + one run on the tiny scene (what smoke() does)
  cloud, mesh                   eval_mesh on 1 000 random points a side; marching_cubes on the tiny TSDF
"""
import ctypes
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cnrma_amd import _lib, cloud, fusion, mesh, pipeline, postprocess, rma, synth  # noqa: E402
from cnrma_amd import nn as snn, sparse as S  # noqa: E402

_call = _lib.call
_TABLE = dict(_lib.SIGNATURES, **_lib.EXPERIMENT_SIGNATURES)


def recorder(name, *args):
    types = _TABLE[name][1]
    assert len(types) == len(args), name
    shown = [("NULL" if not a else "ptr") if t is ctypes.c_void_p else repr(a) for t, a in zip(types, args)]
    print(name, *shown)
    return _call(name, *args)


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


if __name__ == "__main__":
    main()
