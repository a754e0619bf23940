"""What the three graph objects of cnrma_amd.pipeline compute, as hashes: python scripts/static_identity.py > LOG

Builds a StaticScene (dense on, NeuS), a StaticNet (on that scene's aggregated points) and a StaticBatch (B = 2) on tiny synthetic
scenes with a fixed sample_seed, runs each twice and prints one line per output tensor: object, run, name, shape and the SHA-256
of its bytes.  Two trees whose logs are equal launch the same work on the same inputs and get the same bits; the lengths of the
size plans and the node count of the scene graph are printed beside them.  Rows behind a live count are undefined (whatever the
static buffers held), so detections and point coordinates are hashed up to their live counts -- detections() and the count of the
selected points, each one device->host read."""
import hashlib
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cnrma_amd import pipeline, synth  # noqa: E402


def line(obj, run, name, t):
    t = t.detach().cpu().contiguous()
    digest = hashlib.sha256(t.view(torch.uint8).numpy().tobytes() if t.numel() else b"").hexdigest()
    print(f"{obj} run{run} {name} {tuple(t.shape)} {t.dtype} {digest}")


def lines(obj, run, out, b, s):
    line(obj, run, "bboxes", b)
    line(obj, run, "scores", s)
    for name in ("valid", "counts", "status"):
        line(obj, run, name, out[name])


def main():
    from projects.mvsdetection.models.fcaf3d_backbone import FCAF3DBackbone
    from projects.mvsdetection.models.fcaf3d_head import FCAF3DHead
    dev = torch.device("cuda:0")
    scenes = []
    for i in range(2):
        sc = synth.make_scene("tiny", seed=10 + i, boxes=i)
        scenes.append((sc["features"][:, 0].to(dev), sc["projection"][:, 0], sc["tsdf"][0, 0].to(dev),
                       torch.tensor([0.1 * i, -0.2 * i, 0.05])))
    torch.manual_seed(0)
    backbone = FCAF3DBackbone(scenes[0][0].shape[1], 34)
    head = FCAF3DHead(18, (64, 128, 256, 512), 128, 6, 0.01, 1500, None, test_cfg=dict(nms_pre=100))
    backbone.init_weights()
    head.init_weights()
    backbone, head = backbone.to(dev).eval(), head.to(dev).eval()
    cfg = pipeline.SceneConfig(sc["dims"], stride=sc["stride"], max_points=20000, sample_seed=4321, ray_marching_type="neus")

    scene = pipeline.StaticScene(cfg, backbone, head, dev, dense=True)
    for f, p, t, o in scenes:
        scene.calibrate(f, p, t, offset=o)
    plan = scene.plan
    print(f"StaticScene plan sizes {len(plan.sizes)} flags {len(plan.flags)}")
    f, p, t, o = scenes[0]
    scene.build(f, p, t)
    print(f"StaticScene n_nodes {scene.n_nodes} arena_fallbacks {scene.arena_fallbacks}")
    for run in range(2):
        out = scene.run(f, p, t, offset=o)
        b, s, _ = pipeline.StaticScene.detections(out)
        line("StaticScene", run, "volume", out["volume"])
        line("StaticScene", run, "count", out["count"])
        lines("StaticScene", run, out, b, s)
        coords, _, n_sel = out["points"]
        n = int(n_sel)
        line("StaticScene", run, "points", coords[:n])
    pts, pf = coords[:n].clone(), pipeline.StaticScene.point_features(out)[:n].clone()

    net = pipeline.StaticNet(backbone, head, cfg.voxel_size_fcaf3d, dev)
    net.build(pts, pf, cap=n + 1000)
    print(f"StaticNet plan sizes {len(net.plan.sizes)} flags {len(net.plan.flags)}")
    for run in range(2):
        out = net.run(pts, pf)
        b, s, _ = pipeline.StaticScene.detections(out)
        lines("StaticNet", run, out, b, s)

    batch = pipeline.StaticBatch(cfg, backbone, head, dev, 2)
    batch.build(scenes, plan)
    print(f"StaticBatch plan sizes {len(batch.plan.sizes)} flags {len(batch.plan.flags)}")
    for run in range(2):
        out = batch.run(scenes)
        res = batch.detections(out)
        for i, (b, s, _) in enumerate(res):
            line("StaticBatch", run, f"volume[{i}]", out["volume"][i])
            line("StaticBatch", run, f"count[{i}]", out["count"][i])
            line("StaticBatch", run, f"bboxes[{i}]", b)
            line("StaticBatch", run, f"scores[{i}]", s)
        for name in ("valid", "counts", "status"):
            line("StaticBatch", run, name, out[name])


if __name__ == "__main__":
    main()
