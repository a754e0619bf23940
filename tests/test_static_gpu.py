"""The static trace (capacity-sized tensors, device-side row counts, no device->host read) and its HIP-graph replay
must give what the eager path gives: pipeline.StaticScene vs pipeline.forward_scene on the same inputs."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _model(C, dev, n_classes=18, n_reg=6):
    from projects.mvsdetection.models.fcaf3d_backbone import FCAF3DBackbone
    from projects.mvsdetection.models.fcaf3d_head import FCAF3DHead
    torch.manual_seed(0)
    backbone = FCAF3DBackbone(C, 34)
    head = FCAF3DHead(n_classes, (64, 128, 256, 512), 128, n_reg, 0.01, 2000, None, test_cfg=dict(nms_pre=100))
    backbone.init_weights()
    head.init_weights()
    return backbone.to(dev).eval(), head.to(dev).eval()


def _scene(shape, seed, dev, boxes=0):
    from cnrma_amd import synth
    sc = synth.make_scene(shape, seed=seed, boxes=boxes)
    return sc, sc["features"][:, 0].to(dev), sc["projection"][:, 0], sc["tsdf"][0, 0].to(dev)


def _sorted(b, s):
    """rows in a canonical order (levels keep their order; inside a level ties may swap)"""
    key = np.lexsort(tuple(np.round(b[:, i], 4) for i in range(b.shape[1] - 1, -1, -1)))
    return b[key], s[key]


@pytest.mark.parametrize("capture", [False, True])
def test_static_equals_eager_tiny(device, capture):
    from cnrma_amd import pipeline
    sc, feat, proj, tsdf = _scene("tiny", 0, device)
    backbone, head = _model(feat.shape[1], device)
    cfg = pipeline.SceneConfig(sc["dims"], stride=sc["stride"], max_points=20000, sample_seed=1234)
    st = pipeline.StaticScene(cfg, backbone, head, device)
    eager = st.build(feat, proj, tsdf, capture=capture)
    for rep in range(3):                                   # replays must not depend on what the buffers held before
        if rep:
            st.seed_dev.zero_()                            # same point subset as the eager run
        out = st.run(feat, proj, tsdf)
        torch.cuda.synchronize()
        b, s, info = pipeline.StaticScene.detections(out)
        assert info["M"] == eager["M"] and info["M_selected"] == eager["M_selected"] and info["M_unique"] == eager["M_unique"]
        assert info["level_rows"] == eager["level_rows"] and info["head_rows"] == eager["head_rows"]
        assert torch.equal(out["volume"], eager["volume"]) and torch.equal(out["count"], eager["count"])
        assert b.shape == eager["bboxes"].shape
        b0, s0 = _sorted(eager["bboxes"].cpu().numpy(), eager["scores"].cpu().numpy())
        b1, s1 = _sorted(b.cpu().numpy(), s.cpu().numpy())
        # the split over kernel offsets of a short layer depends on its capacity: sums are rounded in another order
        np.testing.assert_allclose(b1, b0, rtol=2e-4, atol=2e-4)
        np.testing.assert_allclose(s1, s0, rtol=2e-4, atol=1e-6)


def test_static_replay_follows_new_inputs(device):
    """a replay on another scene of the same shape = the eager result on that scene"""
    from cnrma_amd import pipeline
    sc, feat, proj, tsdf = _scene("tiny", 0, device)
    backbone, head = _model(feat.shape[1], device)
    cfg = pipeline.SceneConfig(sc["dims"], stride=sc["stride"], max_points=20000, sample_seed=77)
    st = pipeline.StaticScene(cfg, backbone, head, device)
    st.build(feat, proj, tsdf)
    _, feat2, proj2, tsdf2 = _scene("tiny", 5, device)
    st.seed_dev.zero_()
    out = st.run(feat2, proj2, tsdf2)
    torch.cuda.synchronize()
    b, s, info = pipeline.StaticScene.detections(out)
    eager = pipeline.forward_scene(cfg, backbone, head, feat2, proj2, tsdf2)
    assert info["M"] == eager["M"] and info["M_unique"] == eager["M_unique"] and info["level_rows"] == eager["level_rows"]
    assert torch.equal(out["volume"], eager["volume"])
    b0, s0 = _sorted(eager["bboxes"].cpu().numpy(), eager["scores"].cpu().numpy())
    b1, s1 = _sorted(b.cpu().numpy(), s.cpu().numpy())
    np.testing.assert_allclose(b1, b0, rtol=2e-4, atol=2e-4)
    np.testing.assert_allclose(s1, s0, rtol=2e-4, atol=1e-6)


def test_static_flags_a_scene_that_outgrows_the_plan(device):
    """calibrated on an empty room with no margin, then fed a room with furniture (more surface -> more rows): nothing
    may be written out of bounds and the status word must say that the result is invalid"""
    from cnrma_amd import _lib, pipeline
    sc, feat, proj, tsdf = _scene("tiny", 0, device)
    backbone, head = _model(feat.shape[1], device)
    cfg = pipeline.SceneConfig(sc["dims"], stride=sc["stride"], max_points=None, sample_seed=3)
    st = pipeline.StaticScene(cfg, backbone, head, device, margin=1.0)
    st.plan_slack = 0
    st.build(feat, proj, tsdf)
    st.plan.slack = 0
    _, feat2, proj2, tsdf2 = _scene("tiny", 0, device, boxes=6)
    out = st.run(feat2, proj2, tsdf2)
    torch.cuda.synchronize()
    eager = pipeline.forward_scene(cfg, backbone, head, feat2, proj2, tsdf2)
    if eager["M"] > st.plan.sizes[0] + 320:
        with pytest.raises(_lib.CnrmaError):
            pipeline.StaticScene.detections(out)
    # and the object stays usable: the calibration scene still passes
    st.seed_dev.zero_()
    out = st.run(feat, proj, tsdf)
    torch.cuda.synchronize()
    pipeline.StaticScene.detections(out)
    # detect(): the serving call -- falls back to the eager path for the scene that does not fit, static otherwise
    b, s, info = st.detect(feat2, proj2, tsdf2)
    if eager["M"] > st.plan.sizes[0] + 320:
        assert info["static"] is False and st.outgrown is not None
    assert b.shape == eager["bboxes"].shape and info["M"] == eager["M"]
    b, s, info = st.detect(feat, proj, tsdf)
    assert info["static"] is True


def test_static_equals_eager_scannet_shape(device):
    from cnrma_amd import pipeline
    sc, feat, proj, tsdf = _scene("S", 0, device)
    from bench import build_model
    backbone, head = build_model(feat.shape[1], device)
    cfg = pipeline.SceneConfig(sc["dims"], stride=sc["stride"], max_points=500000, sample_seed=99)
    st = pipeline.StaticScene(cfg, backbone, head, device)
    eager = st.build(feat, proj, tsdf)
    # every pre-filled table of the captured trace came from the one arena its sizing run measured (a drift between the two runs
    # would silently cost a clear launch per table: ADVICE round 5), and the graph holds what the bench line reports
    assert st.arena_fallbacks == 0 and st.plan._arena is not None and st.plan._arena_off > 0
    assert st.n_nodes is None or st.n_nodes < 300
    st.seed_dev.zero_()
    out = st.run(feat, proj, tsdf)
    torch.cuda.synchronize()
    b, s, info = pipeline.StaticScene.detections(out)
    assert info["M"] == eager["M"] == 4141048 and info["M_selected"] == 500000 and info["M_unique"] == eager["M_unique"]
    assert info["level_rows"] == eager["level_rows"] and info["head_rows"] == eager["head_rows"]
    assert torch.equal(out["volume"], eager["volume"])
    b0, s0 = _sorted(eager["bboxes"].cpu().numpy(), eager["scores"].cpu().numpy())
    b1, s1 = _sorted(b.cpu().numpy(), s.cpu().numpy())
    # 35 layers deep; rows with near-equal scores can swap ranks at the nms_pre cut: compare the bulk
    close = np.isclose(b1, b0, rtol=5e-4, atol=5e-4).all(axis=1)
    assert close.mean() > 0.99


def test_static_trace_takes_the_pair_list_stem(device):
    """128 input channels: the stem's nearly empty kernel map goes through cnrma_sparse_conv_pairs_f16x3 -- a recorded
    branch of the size plan -- in the calibration run, in the static trace and in the captured graph"""
    from cnrma_amd import pipeline, synth
    from cnrma_amd import sparse as S
    sc = synth.make_scene((3, 128, 30, 40, (48, 48, 20), 4), seed=2)
    feat, proj, tsdf = sc["features"][:, 0].to(device), sc["projection"][:, 0], sc["tsdf"][0, 0].to(device)
    backbone, head = _model(128, device)
    cfg = pipeline.SceneConfig(sc["dims"], stride=sc["stride"], max_points=1500, sample_seed=5)
    calls = []
    orig = S.call
    S.call = lambda name, *a: (calls.append(name), orig(name, *a))[1]
    try:
        st = pipeline.StaticScene(cfg, backbone, head, device)
        eager = st.build(feat, proj, tsdf)
    finally:
        S.call = orig
    assert calls.count("cnrma_sparse_conv_pairs_f16x3") == 3          # calibration, static trace, capture
    assert True in st.plan.flags
    st.seed_dev.zero_()
    out = st.run(feat, proj, tsdf)
    torch.cuda.synchronize()
    b, s, info = pipeline.StaticScene.detections(out)
    assert info["M_unique"] == eager["M_unique"] and info["level_rows"] == eager["level_rows"]
    b0, s0 = _sorted(eager["bboxes"].cpu().numpy(), eager["scores"].cpu().numpy())
    b1, s1 = _sorted(b.cpu().numpy(), s.cpu().numpy())
    np.testing.assert_allclose(b1, b0, rtol=2e-4, atol=2e-4)
    np.testing.assert_allclose(s1, s0, rtol=2e-4, atol=1e-6)


def test_static_equals_eager_north_star_shape(device):
    """the bench workload itself (40 x 256 ch x 480x640 -> 192^3): graph replay vs the eager pass on the same scene --
    same sizes at every level, bit-identical dense volume, the bulk of the detections within 5e-4"""
    from cnrma_amd import pipeline, synth
    from bench import build_model
    if torch.cuda.get_device_properties(0).total_memory < 120e9:
        pytest.skip("needs ~60 GB of device memory")
    sc = synth.make_scene("NS", seed=1, boxes=3, device=device)
    feat, proj, tsdf = sc["features"][:, 0], sc["projection"][:, 0], sc["tsdf"][0, 0].to(device)
    backbone, head = build_model(feat.shape[1], device)
    cfg = pipeline.SceneConfig(sc["dims"], stride=sc["stride"], max_points=500000, sample_seed=7)
    st = pipeline.StaticScene(cfg, backbone, head, device)
    eager = st.build(feat, proj, tsdf)
    st.seed_dev.zero_()
    b, s, info = st.detect(feat, proj, tsdf)
    assert info["static"] is True
    assert info["M"] == eager["M"] and info["M_selected"] == 500000 and info["M_unique"] == eager["M_unique"]
    assert info["level_rows"] == eager["level_rows"] and info["head_rows"] == eager["head_rows"]
    assert torch.equal(st.out["volume"], eager["volume"]) and torch.equal(st.out["count"], eager["count"])
    b0, s0 = _sorted(eager["bboxes"].cpu().numpy(), eager["scores"].cpu().numpy())
    b1, s1 = _sorted(b.cpu().numpy(), s.cpu().numpy())
    assert b1.shape == b0.shape
    close = np.isclose(b1, b0, rtol=5e-4, atol=5e-4).all(axis=1)
    assert close.mean() > 0.99
    del st, eager, feat
    torch.cuda.empty_cache()


@pytest.mark.parametrize("shape,B,max_points", [("tiny", 3, 20000), ("tiny", 2, 700)])
def test_static_batch_equals_single_scenes(device, shape, B, max_points):
    """several scenes per captured pass (pipeline.StaticBatch: per-scene geometric half, ONE collated sparse tensor through
    the network, per-scene instance norm / pruning / decode with device-side counts) = the same scenes one by one through
    the eager path: same row counts at every level per scene, bit-identical dense volumes, detections within 2e-4"""
    from cnrma_amd import pipeline
    scenes = []
    for i in range(B):
        sc, feat, proj, tsdf = _scene(shape, 10 + i, device, boxes=i)
        scenes.append((feat, proj, tsdf, torch.tensor([0.1 * i, -0.2 * i, 0.05])))
    backbone, head = _model(scenes[0][0].shape[1], device)
    head.pts_threshold = 1500 if max_points > 1000 else 200000          # the first case prunes, the second does not
    cfg = pipeline.SceneConfig(sc["dims"], stride=sc["stride"], max_points=max_points, sample_seed=4321)
    cal = pipeline.StaticScene(cfg, backbone, head, device)
    eager = [cal.calibrate(f, p, t, offset=o) for f, p, t, o in scenes]
    batch = pipeline.StaticBatch(cfg, backbone, head, device, B)
    batch.build(scenes, cal.plan)
    assert batch.graph is not None
    batch.run(list(reversed(scenes)))                                     # other inputs through the graph first
    out = batch.run(scenes)
    res = batch.detections(out)
    for b, ((bb, ss, info), e) in enumerate(zip(res, eager)):
        assert info["M"] == e["M"] and info["M_selected"] == e["M_selected"] and info["M_unique"] == e["M_unique"], (b, info, e["M"])
        assert info["level_rows"] == e["level_rows"] and info["head_rows"] == e["head_rows"], (b, info, e["level_rows"], e["head_rows"])
        assert torch.equal(out["volume"][b], e["volume"]) and torch.equal(out["count"][b], e["count"])
        assert bb.shape == e["bboxes"].shape
        b0, s0 = _sorted(e["bboxes"].cpu().numpy(), e["scores"].cpu().numpy())
        b1, s1 = _sorted(bb.cpu().numpy(), ss.cpu().numpy())
        np.testing.assert_allclose(b1, b0, rtol=2e-4, atol=2e-4)
        np.testing.assert_allclose(s1, s0, rtol=2e-4, atol=1e-6)


def test_detect_recaptures_after_repeated_plan_violations(device):
    """a deployment whose scenes outgrow the calibrated plan (here: a plan deliberately shrunk to a quarter of the recorded
    sizes): detect() serves them through the eager path, keeps their sizes and -- after `rebuild_after` of them --
    enlarges the plan and captures the graph again, so that the same scenes run statically afterwards (ADVICE round 2:
    the outgrown sizes used to be collected and never used)"""
    from cnrma_amd import pipeline
    sc, feat, proj, tsdf = _scene("tiny", 0, device, boxes=4)
    backbone, head = _model(feat.shape[1], device)
    cfg = pipeline.SceneConfig(sc["dims"], stride=sc["stride"], max_points=None, sample_seed=3)
    st = pipeline.StaticScene(cfg, backbone, head, device, margin=1.0)
    eager = st.calibrate(feat, proj, tsdf)
    true_sizes = list(st.plan.sizes)
    st.plan.sizes = [max(1, n // 4) for n in true_sizes]
    st.plan.slack = 0
    st.build(feat, proj, tsdf)
    seen = []
    for i in range(3):
        b, s, info = st.detect(feat, proj, tsdf, rebuild_after=3)
        seen.append((info["static"], info.get("rebuilt", False)))
        assert b.shape == eager["bboxes"].shape and info["M"] == eager["M"]
    assert seen == [(False, False), (False, False), (False, True)]
    assert st.plan.sizes == true_sizes and st.outgrown is None
    b, s, info = st.detect(feat, proj, tsdf, rebuild_after=3)
    assert info["static"] is True and info["M"] == eager["M"] and b.shape == eager["bboxes"].shape
    b0, s0 = _sorted(eager["bboxes"].cpu().numpy(), eager["scores"].cpu().numpy())
    b1, s1 = _sorted(b.cpu().numpy(), s.cpu().numpy())
    np.testing.assert_allclose(b1, b0, rtol=2e-4, atol=2e-4)


@pytest.mark.parametrize("k", [0, 1, 2])
def test_static_depth_mode_vs_reference_golden(device, k):
    """ray_projection_depth (ray_marching.py:809-956; `ray_marching_type='depth'`, depth_points = k) inside the static trace /
    graph -- row count on the device, capacity-guarded emission -- against the reference's golden depth rows of the fixture
    scene: places bit-exact, aggregated features (f * w / mean(w)) within 1e-6; row counts and detections equal to the eager
    path's"""
    from helpers import load_golden, t
    from cnrma_amd import pipeline
    g = load_golden("mini_p")
    # the fixture holds the reference's depth rows of view 0: a one-view scene
    feat, proj, tsdf, pinv = t(g["features"][:1], device), t(g["projection"][:1]), t(g["tsdf"], device), t(g["proj_inv"][:1])
    backbone, head = _model(feat.shape[1], device)
    cfg = pipeline.SceneConfig(g["dims"], voxel_size=g["voxel_size"], origin=g["origin"], stride=g["stride"],
                               n_steps=g["n_steps"], max_points=20000, sample_seed=9, ray_marching_type="depth", depth_points=k)
    st = pipeline.StaticScene(cfg, backbone, head, device)
    eager = st.build(feat, proj, tsdf, proj_inv=pinv)
    assert st.graph is not None and st.march is None
    st.run(feat * 0.5, proj, tsdf * 0.7, proj_inv=pinv)                  # other inputs through the graph first
    out = st.run(feat, proj, tsdf, proj_inv=pinv)
    b, s, info = pipeline.StaticScene.detections(out)
    exp = g[f"depth_rows_k{k}"]
    n = exp.shape[0]
    assert info["M"] == eager["M"] == n > 0 and info["M_unique"] == eager["M_unique"]
    assert info["level_rows"] == eager["level_rows"] and info["head_rows"] == eager["head_rows"]
    coords, _, n_sel = out["points"]
    pf = pipeline.StaticScene.point_features(out)
    assert int(n_sel) == n
    assert (coords[:n].cpu().numpy().view(np.uint32) == exp[:, :3].astype(np.float32).view(np.uint32)).all()
    w = exp[:, 3].astype(np.float64)
    want = exp[:, 4:] * (exp[:, 3:4] / np.float32(w.sum() / n))
    np.testing.assert_allclose(pf[:n].cpu().numpy(), want, rtol=2e-6, atol=1e-7)
    b0, s0 = _sorted(eager["bboxes"].cpu().numpy(), eager["scores"].cpu().numpy())
    b1, s1 = _sorted(b.cpu().numpy(), s.cpu().numpy())
    np.testing.assert_allclose(b1, b0, rtol=2e-4, atol=2e-4)
    np.testing.assert_allclose(s1, s0, rtol=2e-4, atol=1e-6)


@pytest.mark.parametrize("shape", ["tiny", "S"])
def test_channels_last_maps_are_read_in_place_with_identical_results(device, shape):
    """feature maps that are channels-last IN MEMORY (what the plugin's 2D stack hands over) reach the kernels by reference
    (cnrma_backproject_accum_ref_f32 / cnrma_rma_neus_emit_rows_ref_f32): no layout pass, no copy into the slot -- and bit
    for bit the results of the NCHW hand-off (ray_marching.py:211-244: the values are the same, only the strides differ);
    the slot's own channels-last buffer is never allocated, and scenes of both layouts can alternate on one graph"""
    from cnrma_amd import pipeline, rma
    sc, feat, proj, tsdf = _scene(shape, 3, device, boxes=2)
    sc2, feat2, proj2, tsdf2 = _scene(shape, 4, device, boxes=1)
    backbone, head = _model(feat.shape[1], device)
    cfg = pipeline.SceneConfig(sc["dims"], stride=sc["stride"], max_points=20000 if shape == "tiny" else 500000, sample_seed=77)
    cl = feat.contiguous(memory_format=torch.channels_last)
    cl2 = feat2.contiguous(memory_format=torch.channels_last)
    assert rma.is_channels_last(cl) and not rma.is_channels_last(feat) and torch.equal(cl, feat)
    st = pipeline.StaticScene(cfg, backbone, head, device)
    st.build(cl, proj, tsdf)
    assert st.graph is not None and st.nhwc is None                      # built and captured without a channels-last copy

    def run(f, p, t):
        out = st.run(f, p, t)
        b, s, info = pipeline.StaticScene.detections(out)
        n = int(out["points"][2])                                         # rows behind the live count are undefined
        return (out["volume"].clone(), out["count"].clone(), out["points"][0][:n].clone(),
                pipeline.StaticScene.point_features(out)[:n].clone(), b.clone(), s.clone(), info)
    a = run(cl, proj, tsdf)
    assert st.nhwc is None
    other = run(cl2, proj2, tsdf2)                                        # another producer tensor: only the reference changes
    b = run(feat, proj, tsdf)                                             # NCHW on the same graph: layout pass into the slot's buffer
    assert st.nhwc is not None
    c = run(cl, proj, tsdf)
    for x, y, z in zip(a[:6], b[:6], c[:6]):
        assert torch.equal(x, y) and torch.equal(x, z)
    assert a[6] == b[6] == c[6]
    assert not torch.equal(a[0], other[0])
    eager = pipeline.forward_scene(cfg, backbone, head, cl, proj, tsdf)
    assert torch.equal(eager["volume"], a[0]) and torch.equal(eager["count"], a[1])


def test_copy_hand_off_lets_the_producer_overwrite_its_buffer(device):
    """reading channels-last maps in place is a contract (nobody writes them until out["done"]); a producer
    that reuses its output buffer asks for by_reference=False: the maps are copied into the slot's buffer, the caller may
    overwrite its tensor once out["inputs_consumed"] has completed, and the results are those of the reference hand-off."""
    from cnrma_amd import pipeline
    sc, feat, proj, tsdf = _scene("tiny", 3, device, boxes=2)
    backbone, head = _model(feat.shape[1], device)
    cfg = pipeline.SceneConfig(sc["dims"], stride=sc["stride"], max_points=20000, sample_seed=77)
    cl = feat.contiguous(memory_format=torch.channels_last)
    st = pipeline.StaticScene(cfg, backbone, head, device)
    st.build(cl, proj, tsdf)
    out = st.run(cl, proj, tsdf)
    assert st._held is cl and out["inputs_consumed"] is out["done"]      # by reference: free again only after the scene
    b0, s0, _ = pipeline.StaticScene.detections(out)
    vol0, b0, s0 = out["volume"].clone(), b0.clone(), s0.clone()
    buf = cl.clone(memory_format=torch.channels_last)                    # a producer-owned, reused output buffer
    out = st.run(buf, proj, tsdf, by_reference=False)
    assert st._held is None and st.nhwc is not None and out["inputs_consumed"] is not out["done"]
    out["inputs_consumed"].synchronize()
    buf.zero_()                                                          # the producer's next output lands in the same memory
    b1, s1, _ = pipeline.StaticScene.detections(out)
    assert torch.equal(out["volume"], vol0) and torch.equal(b1, b0) and torch.equal(s1, s0)
    # slot-level default
    st2 = pipeline.StaticScene(cfg, backbone, head, device, by_reference=False)
    st2.build(cl, proj, tsdf, plan=st.plan)
    out2 = st2.run(cl, proj, tsdf)
    assert st2._held is None
    b2, s2, _ = pipeline.StaticScene.detections(out2)
    assert torch.equal(out2["volume"], vol0) and torch.equal(b2, b0) and torch.equal(s2, s0)


# ---------------------------------------------------------------------------------------------------------------------
# the lifecycle the three graph objects share: traced without capture, an outgrown plan, ordering behind the producer
# ---------------------------------------------------------------------------------------------------------------------
_BATCH_CASE = {}


def _batch_case(device):
    """two tiny scenes, the small model, their calibrated single-scene plan and what the CAPTURED batch returns for them
    (out, detections): computed once, read by the tests below and left unchanged"""
    if not _BATCH_CASE:
        from cnrma_amd import pipeline
        scenes = []
        for i in range(2):
            sc, feat, proj, tsdf = _scene("tiny", 10 + i, device, boxes=i)
            scenes.append((feat, proj, tsdf, torch.tensor([0.1 * i, -0.2 * i, 0.05])))
        backbone, head = _model(scenes[0][0].shape[1], device)
        head.pts_threshold = 1500
        cfg = pipeline.SceneConfig(sc["dims"], stride=sc["stride"], max_points=20000, sample_seed=4321)
        cal = pipeline.StaticScene(cfg, backbone, head, device)
        for f, p, t, o in scenes:
            cal.calibrate(f, p, t, offset=o)
        batch = pipeline.StaticBatch(cfg, backbone, head, device, 2)
        batch.build(scenes, cal.plan)
        assert batch.graph is not None
        out = batch.run(scenes)
        res = batch.detections(out)
        ref = dict(volume=[v.clone() for v in out["volume"]], count=[c.clone() for c in out["count"]],
                   dets=[(b.clone(), s.clone(), info) for b, s, info in res])
        _BATCH_CASE.update(scenes=scenes, model=(backbone, head), cfg=cfg, plan=cal.plan, ref=ref)
    return _BATCH_CASE


def _assert_batch_equals_reference(out, res, ref):
    for i, ((b, s, info), (b0, s0, info0)) in enumerate(zip(res, ref["dets"])):
        assert info == info0, (i, info, info0)
        assert torch.equal(out["volume"][i], ref["volume"][i]) and torch.equal(out["count"][i], ref["count"][i])
        assert torch.equal(b, b0) and torch.equal(s, s0)


def test_static_batch_traced_without_capture_equals_the_captured_batch(device):
    """capture=False: run() goes through the launch sequence itself instead of a graph replay -- the same kernels on the same
    capacities, so the same bits: info, dense volumes and counts, boxes and scores of both scenes"""
    from cnrma_amd import pipeline
    case = _batch_case(device)
    batch = pipeline.StaticBatch(case["cfg"], *case["model"], device, 2)
    batch.build(case["scenes"], case["plan"], capture=False)
    assert batch.graph is None
    batch.run(list(reversed(case["scenes"])))                            # other inputs through the trace first
    out = batch.run(case["scenes"])
    _assert_batch_equals_reference(out, batch.detections(out), case["ref"])


def test_static_batch_flags_scenes_that_outgrow_the_plan(device):
    """a plan cut to a quarter of the calibrated sizes (no slack, no margin): every kernel of the pass stays inside its
    capacities, detections() raises, and another batch on the true plan serves the same scenes with the same results"""
    from cnrma_amd import _lib, pipeline
    from cnrma_amd import plan as P
    case = _batch_case(device)
    small = P.Plan(1.0, 0)
    small.sizes = [max(1, n // 4) for n in case["plan"].sizes]
    small.flags, small.marks = list(case["plan"].flags), dict(case["plan"].marks)
    batch = pipeline.StaticBatch(case["cfg"], *case["model"], device, 2)
    batch.build(case["scenes"], small)
    out = batch.run(case["scenes"])
    with pytest.raises(_lib.CnrmaError):
        batch.detections(out)
    torch.cuda.synchronize()
    good = pipeline.StaticBatch(case["cfg"], *case["model"], device, 2)
    good.build(case["scenes"], case["plan"])
    out = good.run(case["scenes"])
    _assert_batch_equals_reference(out, good.detections(out), case["ref"])


@pytest.mark.parametrize("kind", ["net", "batch"])
def test_net_and_batch_order_themselves_behind_the_producer_stream(device, kind):
    """what test_run_orders_itself_behind_the_producer_stream (test_static_oracle_gpu.py) checks for StaticScene, for the other
    two graph objects: inputs written late on the caller's stream, right before run(), and freed right after it"""
    from cnrma_amd import pipeline
    case = _batch_case(device)
    backbone, head = case["model"]
    if kind == "batch":
        obj = pipeline.StaticBatch(case["cfg"], backbone, head, device, 2)
        obj.build(case["scenes"], case["plan"])
        inputs = [case["scenes"][0][0], case["scenes"][1][0]]                # the two scenes' feature maps

        def run(fresh):
            out = obj.run([(f,) + sc_[1:] for f, sc_ in zip(fresh, case["scenes"])])
            return out, lambda: [r[0] for r in obj.detections(out)] + list(out["volume"])
    else:
        rng = np.random.RandomState(3)
        pts = rng.rand(6000, 3).astype(np.float32) * np.array([1.0, 0.8, 0.6], dtype=np.float32)
        pts[:2000, 2] = 0.01 * rng.rand(2000)                                # a floor and a wall: surfaces, like a scene
        pts[2000:4000, 0] = 1.0 - 0.01 * rng.rand(2000)
        C = case["scenes"][0][0].shape[1]
        inputs = [torch.from_numpy(pts).to(device), torch.from_numpy(rng.randn(6000, C).astype(np.float32)).to(device)]
        obj = pipeline.StaticNet(backbone, head, 0.01, device)
        obj.build(*inputs)

        def run(fresh):
            out = obj.run(*fresh)
            return out, lambda: [pipeline.StaticScene.detections(out)[0]]
    assert obj.graph is not None
    _, read = run(inputs)
    torch.cuda.synchronize()
    ref = [t.clone() for t in read()]
    big = torch.randn(4096, 4096, device=device)
    for _ in range(3):
        junk = big @ big                                       # keeps the default stream busy for a while
        fresh = [(x * 3.0 / 3.0 * 1.0 + junk[0, 0] * 0.0) for x in inputs]
        fresh = [(x + (y - y)).contiguous() for x, y in zip(inputs, fresh)]     # == inputs, but fresh allocations written just now
        _, read = run(fresh)
        del fresh                                              # the allocator may hand the blocks out again right away
        scratch = [torch.full_like(x, 7.0) for x in inputs]
        got = read()
        assert len(got) == len(ref) and all(torch.equal(a, b) for a, b in zip(got, ref))
        del scratch
