"""GPU tests (-m gpu) of the 16-bit feature-map path: the dense unprojection, the NeuS row emission, the layout pass, the static
slot and the plugin on fp16 / bf16 maps read where they lie.

fp16 -> fp32 and bf16 -> fp32 are exact and every sum stays fp32 in view order, so there is ONE bar everywhere: bit equality
with the fp32 path (and, for the dense kernel, with the oracle) fed the same maps widened with `.float()`.  No tolerance
appears in this file.  The maps carry finite specials of their type -- its largest finite value, its smallest subnormal, -0.0
and a value with all mantissa bits set -- in pixels that voxels and rays do see."""
import os
import runpy

import numpy as np
import pytest
import torch

from oracle import rma_oracle as O

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = [torch.float16, torch.bfloat16]
IDS = ["fp16", "bf16"]
ELEM = {torch.float16: 1, torch.bfloat16: 2}


def _specials(dtype):
    """largest finite value, smallest subnormal, -0.0, all mantissa bits set (exponent of 1.0) -- as exact fp32 values"""
    fi = torch.finfo(dtype)
    mant = 10 if dtype == torch.float16 else 7
    return torch.tensor([fi.max, fi.smallest_normal * 2.0 ** -mant, -0.0, 2.0 - 2.0 ** -mant], dtype=torch.float32)


def _plant(feat, dtype, network=False):
    """feat [V,C,H,W] fp32 -> the 16-bit maps with specials planted in every 7th pixel of every view (all channels; the four
    values cycle over pixel and channel).  Only +max is planted, so sums may reach +inf but never inf - inf.
    network=True (the tests that run the sparse network behind the geometric half): bf16 maps leave the largest finite value
    out -- it is 3.4e38 = fp32's own largest value less 7 mantissa bits, so a point feature max * w / mean(w) is +inf as soon
    as a ray weight is above the mean, the network turns that into NaN, and NaN != NaN would fail an equality that has nothing
    to do with how the maps are read.  fp16 maps keep theirs: 65504 * w / mean(w) with weights in [threshold, 1] stays below
    65504 / threshold, some thirty orders of magnitude short of fp32's range, and so do the network's sums of squares."""
    V, C, H, W = feat.shape
    sp = _specials(dtype)
    if network and dtype == torch.bfloat16:
        sp[0] = sp[3]
    f = feat.clone().view(V, C, H * W)
    pix = torch.arange(0, H * W, 7)
    which = (pix.view(1, 1, -1) // 7 + torch.arange(C).view(1, C, 1) + torch.arange(V).view(V, 1, 1)) % 4
    f[:, :, pix] = sp[which]
    h = f.view(V, C, H, W).to(dtype)
    assert torch.equal(h.view(V, C, H * W)[:, :, pix].float(), sp[which])          # the cast kept them exactly
    return h


def _scene(V, C, dims, seed, dtype, blind_view=True):
    """small maps (30 x 40, stride 4) around `dims`, as tests/test_dense_store_runs_gpu.py builds them"""
    from cnrma_amd import synth
    sc = synth.make_scene((V, C, 30, 40, tuple(dims), 4), seed=seed)
    feat, proj = sc["features"][:, 0], sc["projection"][:, 0].clone()
    if blind_view:
        proj[V // 2, 2] = torch.tensor([0.0, 0.0, 0.0, -1.0])        # depth -1 for every voxel: the view adds nothing anywhere
    return _plant(feat, dtype), proj, sc


def _bits(t):
    return t.contiguous().view(torch.int32)


def _launch(entry, feat_nhwc, proj_scaled, dims, by_ref, offset_floats, device):
    """one C entry point ("h16" | "f32") with an output volume that starts `offset_floats` floats into a NaN-filled buffer;
    returns the volume, the count and the buffer's guard words (which must stay NaN)"""
    from cnrma_amd import rma
    from cnrma_amd._lib import call, ptr, stream
    V, H, W, C = feat_nhwc.shape
    X, Y, Z = dims
    G = X * Y * Z
    buf = torch.full((C * G + 8,), float("nan"), dtype=torch.float32, device=device)
    volume = buf[offset_floats:offset_floats + C * G]
    count = torch.full((G,), -7, dtype=torch.int32, device=device)
    st = stream()
    ws = rma._dense_workspace(device, st)
    tail = (ptr(proj_scaled), V, C, H, W, X, Y, Z, 0.04, 0.0, 0.0, 0.0, ptr(volume), ptr(count), ptr(ws), ws.numel() * 4, st)
    ref = torch.tensor([feat_nhwc.data_ptr()], dtype=torch.int64, device=device)
    if entry == "h16":
        call("cnrma_backproject_accum_h16", None if by_ref else ptr(feat_nhwc), ptr(ref) if by_ref else None,
             ELEM[feat_nhwc.dtype], *tail)
    elif by_ref:
        call("cnrma_backproject_accum_ref_f32", ptr(ref), *tail)
    else:
        call("cnrma_backproject_accum_f32", ptr(feat_nhwc), *tail)
    torch.cuda.synchronize()
    guards = torch.cat((buf[:offset_floats], buf[offset_floats + C * G:]))
    return volume.view(C, X, Y, Z).cpu(), count.view(X, Y, Z).cpu(), guards.cpu()


def _check_dense(V, C, dims, seed, dtype, device, offsets=(0,)):
    from cnrma_amd import rma
    h, proj, sc = _scene(V, C, dims, seed, dtype)
    vol, cnt = O.backproject_accum(dims, 0.04, (0.0, 0.0, 0.0), proj, h.float(), 4)
    assert int(cnt.max()) > 1                                        # voxels that several views see exist
    assert float(vol.max()) >= float(torch.finfo(dtype).max) / V     # ... and planted pixels are among what they see
    nhwc = rma.to_nhwc(h.to(device), keep_dtype=True)
    assert nhwc.dtype == dtype
    wide = nhwc.float()
    ps = rma.scale_projection(proj, 4).to(device)
    for off in offsets:
        for by_ref in (False, True):
            gv, gc, guards = _launch("h16", nhwc, ps, dims, by_ref, off, device)
            tag = (dims, C, off, by_ref, dtype)
            assert torch.isnan(guards).all(), tag
            assert torch.equal(gc.long(), cnt), tag
            assert torch.equal(_bits(gv), _bits(vol)), tag                           # the oracle on h.float()
            fv, fc, _ = _launch("f32", wide, ps, dims, by_ref, off, device)       # the existing fp32 entry points on h.float()
            assert torch.equal(gc, fc) and torch.equal(_bits(gv), _bits(fv)), tag


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("C", [8, 16, 32, 64, 128])
def test_dense_every_lane_shape(device, C, dtype):
    """1, 2 and 4 lanes per voxel (C = 8, 16, 32) and two and four channel sweeps (C = 64, 128), on a grid with whole and broken
    z-runs and on one smaller than a brick"""
    _check_dense(3, C, (24, 20, 36), 20 + C, dtype, device)
    _check_dense(3, C, (10, 12, 7), 40 + C, dtype, device)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("Z", [5, 8, 33])
def test_dense_broken_and_whole_z_runs(device, Z, dtype):
    _check_dense(4, 64, (20, 18, Z), 10 + Z, dtype, device)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_dense_grid_size_not_a_multiple_of_4(device, dtype):
    assert (9 * 7 * 5) % 4 != 0
    _check_dense(3, 32, (9, 7, 5), 3, dtype, device)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_dense_more_than_one_brick_ragged(device, dtype):
    _check_dense(3, 32, (40, 36, 44), 5, dtype, device)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_dense_volume_at_an_offset_into_a_guarded_buffer(device, dtype):
    """the output is a view 1 and 4 floats into a NaN-filled buffer: element stores and 16-byte stores, the guard words stay NaN"""
    _check_dense(3, 32, (20, 18, 8), 7, dtype, device, offsets=(1, 4))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_dense_host_falls_back_for_maps_the_kernel_cannot_load(device, dtype):
    """C = 12, and a map tensor that starts 2 bytes into its storage: rma.backproject_accum widens them and is still bit-equal"""
    from cnrma_amd import rma
    dims = (20, 18, 8)
    for C, shifted in ((12, False), (16, True)):
        h, proj, _ = _scene(3, C, dims, 60 + C, dtype)
        vol, cnt = O.backproject_accum(dims, 0.04, (0.0, 0.0, 0.0), proj, h.float(), 4)
        assert int(cnt.max()) > 1
        nhwc = h.permute(0, 2, 3, 1).contiguous().to(device)
        if shifted:
            flat = torch.empty(nhwc.numel() + 8, dtype=dtype, device=device)
            view = flat[1:1 + nhwc.numel()].view(nhwc.shape)
            view.copy_(nhwc)
            nhwc = view
            assert nhwc.data_ptr() % 16 == 2 and nhwc.is_contiguous()
        gv, gc = rma.backproject_accum(nhwc, proj, dims, 0.04, (0.0, 0.0, 0.0), 4)
        assert torch.equal(gc.cpu().long(), cnt) and torch.equal(_bits(gv.cpu()), _bits(vol)), (C, shifted)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_dense_both_c64_forms_agree(device, dtype):
    """the experiments library carries both C % 64 == 0 forms (4 and 8 lanes per voxel): each equals the product library"""
    from cnrma_amd import rma
    dims = (24, 20, 36)
    for C in (64, 128):
        h, proj, _ = _scene(3, C, dims, 80 + C, dtype)
        nhwc = rma.to_nhwc(h.to(device), keep_dtype=True)
        vol, cnt = rma.backproject_accum(nhwc, proj, dims, 0.04, (0.0, 0.0, 0.0), 4)
        assert int(cnt.max()) > 1
        try:
            for lanes in (4, 8):
                rma.dense_tuning(lpv=lanes)
                v2, c2 = rma.backproject_accum(nhwc, proj, dims, 0.04, (0.0, 0.0, 0.0), 4)
                assert torch.equal(c2, cnt) and torch.equal(_bits(v2), _bits(vol)), (C, lanes)
        finally:
            rma.dense_tuning()


# ---- layout pass ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("hw", [(30, 40), (5, 7)])
@pytest.mark.parametrize("C", [8, 32, 64, 6])
def test_layout_pass_16_bit(device, C, hw, dtype):
    """H * W = 1200 with C % 8 == 0 takes the 16-byte kernel, everything else the element kernel; the elements behind the output
    stay untouched"""
    from cnrma_amd import rma
    H, W = hw
    g = torch.Generator().manual_seed(C * 100 + H)
    x = torch.randn(2, C, H, W, generator=g).to(dtype).to(device)
    n = x.numel()
    buf = torch.full((n + 16,), 123.0, dtype=dtype, device=device)
    out = buf[:n].view(2, H, W, C)
    got = rma.to_nhwc(x, out=out, keep_dtype=True)
    assert got.data_ptr() == buf.data_ptr() and got.dtype == dtype
    assert torch.equal(got.view(torch.int16), x.permute(0, 2, 3, 1).contiguous().view(torch.int16))
    assert torch.equal(buf[n:], torch.full((16,), 123.0, dtype=dtype, device=device))
    fresh = rma.to_nhwc(x, keep_dtype=True)                                 # allocated here
    assert fresh.dtype == dtype and torch.equal(fresh.view(torch.int16), got.view(torch.int16))
    cl = x.contiguous(memory_format=torch.channels_last)
    assert rma.is_channels_last(cl, (dtype,)) and not rma.is_channels_last(cl)
    assert rma.to_nhwc(cl, keep_dtype=True).data_ptr() == cl.data_ptr()      # channels-last in memory: a view
    assert rma.to_nhwc(cl).dtype == torch.float32                            # the default still widens


# ---- NeuS row emission ------------------------------------------------------------------------------------------------------
def _march_scene(C, dtype, device, seed=3):
    from cnrma_amd import rma, synth
    sc = synth.make_scene((3, C, 30, 40, (48, 48, 20), 4), seed=seed, boxes=2)
    h = _plant(sc["features"][:, 0], dtype)
    nhwc = h.permute(0, 2, 3, 1).contiguous().to(device)
    pinv = rma.projection_inverse(sc["projection"][:, 0], 4).to(device)
    return sc, nhwc, pinv, sc["tsdf"][0, 0].to(device)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("C", [8, 12, 32, 256])
def test_aggregate_points_on_16_bit_maps(device, C, dtype):
    """C = 12: widened by the host (element-wise fp32 path); 8, 32, 256: the 2-, 8- and 64-lane-per-row 16-bit kernels.  Once
    every row is kept, once the device sampler cuts"""
    from cnrma_amd import rma
    sc, nhwc, pinv, tsdf = _march_scene(C, dtype, device)
    wide = nhwc.float()
    M = None
    for cut in (False, True):
        mp = None if not cut else max(1, M // 3)
        kw = dict(n_steps=300, thr=0.05, mode="neus", offset=(0.25, -0.5, 0.125), max_points=mp, sampler="device", seed=1234)
        c16, f16, i16 = rma.aggregate_points(nhwc, pinv, tsdf, sc["dims"], 0.04, sc["origin"], **kw)
        c32, f32, i32 = rma.aggregate_points(wide, pinv, tsdf, sc["dims"], 0.04, sc["origin"], **kw)
        M = i32["M"]
        assert c16.shape[0] > 0 and i16["M"] == M and i16["M_selected"] == i32["M_selected"] == c16.shape[0]
        assert (c16.shape[0] < M) == cut
        assert f16.dtype == torch.float32 and torch.equal(_bits(c16), _bits(c32)) and torch.equal(_bits(f16), _bits(f32))
        for k in ("mean_w", "row_offset", "count"):                        # (`kept` has undefined slots behind every ray's count)
            assert torch.equal(i16[k], i32[k]), k
        assert (i16["sel"] is None) == (i32["sel"] is None) and (i16["sel"] is None or torch.equal(i16["sel"], i32["sel"]))
        assert i16["march"].elem == (ELEM[dtype] if C % 8 == 0 else 0)
        assert float(f16.abs().max()) >= 1.0                                # features arrived


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_row_emission_element_path(device, dtype):
    """an output row stride that is no multiple of 4 floats: the 16-bit kernel emits element by element, and the column behind
    every row stays untouched"""
    from cnrma_amd import rma
    C = 8
    sc, nhwc, pinv, tsdf = _march_scene(C, dtype, device)
    outs = []
    for maps in (nhwc, nhwc.float()):
        m = rma._March(maps, pinv, tsdf, sc["dims"], 0.04, sc["origin"], 300, 0.05, "neus", 0)
        cnt, wsum, kept, overflow = m.march()
        off = rma.exclusive_scan(cnt)
        M = int(off[-1].item())
        assert M > 0 and int(overflow.item()) == 0
        rows = torch.full((M, C + 1), float("nan"), dtype=torch.float32, device=device)
        xyz = torch.empty((M, 3), dtype=torch.float32, device=device)
        m.emit_rows(off, M, kept, None, None, (0.0, 0.0, 0.0), xyz.data_ptr(), 3, None, 0, rows.data_ptr(), C + 1)
        torch.cuda.synchronize()
        outs.append((rows, xyz, m.elem))
    assert outs[0][2] == ELEM[dtype] and outs[1][2] == 0
    assert torch.isnan(outs[0][0][:, C]).all()
    assert torch.equal(_bits(outs[0][0][:, :C]), _bits(outs[1][0][:, :C])) and torch.equal(outs[0][1], outs[1][1])


# ---- static slot --------------------------------------------------------------------------------------------------------
def _model(C, dev, n_classes=18, n_reg=6):
    from projects.mvsdetection.models.fcaf3d_backbone import FCAF3DBackbone
    from projects.mvsdetection.models.fcaf3d_head import FCAF3DHead
    torch.manual_seed(0)
    backbone = FCAF3DBackbone(C, 34)
    head = FCAF3DHead(n_classes, (64, 128, 256, 512), 128, n_reg, 0.01, 2000, None, test_cfg=dict(nms_pre=100))
    backbone.init_weights()
    head.init_weights()
    return backbone.to(dev).eval(), head.to(dev).eval()


def _tiny(seed, dtype, dev, boxes):
    from cnrma_amd import synth
    sc = synth.make_scene("tiny", seed=seed, boxes=boxes)
    h = _plant(sc["features"][:, 0], dtype, network=True).to(dev)
    return sc, h, sc["projection"][:, 0], sc["tsdf"][0, 0].to(dev)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_static_slot_reads_16_bit_maps_in_place(device, dtype):
    """a fp32 slot on h.float() and a 16-bit slot of the same plan on h: every output of a replay is torch.equal; NCHW 16-bit maps go
    through the 16-bit layout pass into a buffer of half the size; fp32 maps are refused"""
    from cnrma_amd import pipeline
    sc, h, proj, tsdf = _tiny(3, dtype, device, 2)
    _, h2, proj2, tsdf2 = _tiny(4, dtype, device, 1)
    backbone, head = _model(h.shape[1], device)
    cfg = pipeline.SceneConfig(sc["dims"], stride=sc["stride"], max_points=20000, sample_seed=77)
    cl, cl2 = h.contiguous(memory_format=torch.channels_last), h2.contiguous(memory_format=torch.channels_last)
    wide = h.float().contiguous(memory_format=torch.channels_last)

    def run(st, f, p, t):
        out = st.run(f, p, t)
        b, s, info = pipeline.StaticScene.detections(out)
        n = int(out["points"][2])                                         # rows behind the live count are undefined
        assert n > 0
        return (out["volume"].clone(), out["count"].clone(), out["points"][0][:n].clone(),
                pipeline.StaticScene.point_features(out)[:n].clone(), b.clone(), s.clone(), info)
    st32 = pipeline.StaticScene(cfg, backbone, head, device)
    st32.build(wide, proj, tsdf)
    ref = run(st32, wide, proj, tsdf)
    assert int(ref[1].max()) > 1
    st = pipeline.StaticScene(cfg, backbone, head, device, feature_dtype=dtype)
    st.build(cl, proj, tsdf, plan=st32.plan)
    assert st.graph is not None and st.nhwc is None and st.march.elem == ELEM[dtype]
    a = run(st, cl, proj, tsdf)
    assert st.nhwc is None                                                # read in place: no buffer of the slot's own
    for x, y in zip(ref[:6], a[:6]):
        assert torch.equal(x, y)
    assert ref[6] == a[6]
    b = run(st, h, proj, tsdf)                                            # NCHW 16-bit maps on the same graph
    assert st.nhwc is not None and st.nhwc.dtype == dtype
    assert st.nhwc.numel() * st.nhwc.element_size() * 2 == wide.numel() * 4      # half of what the fp32 slot's buffer would take
    for x, y in zip(a[:6], b[:6]):
        assert torch.equal(x, y)
    other = run(st, cl2, proj2, tsdf2)                                    # another scene, channels-last again
    assert not torch.equal(a[0], other[0]) and not torch.equal(a[3][:8], other[3][:8])
    with pytest.raises(ValueError):
        st.run(wide, proj, tsdf)
    eager = pipeline.forward_scene(cfg, backbone, head, cl, proj, tsdf, keep_half=True)
    assert torch.equal(eager["volume"], a[0]) and torch.equal(eager["count"], a[1])


# ---- plugin ---------------------------------------------------------------------------------------------------------------
def _detector(tmp_path, dims, device, **kw):
    import projects.mvsdetection  # noqa: F401
    from projects.mvsdetection.registry import build_model
    cfg = runpy.run_path(os.path.join(ROOT, "projects", "configs", "mvsdetection", "ray_marching_scannet.py"))
    m = dict(cfg["model"])
    m.update(backbone2d=None, feature_2d=None, backbone_3d=None, tsdf_head=None)      # hot path only: features / TSDF come in
    m.update(save_path=str(tmp_path / "results"), voxel_dim_test=list(dims), voxel_dim_train=list(dims), max_points=100000)
    m.update(kw)
    m["detection_backbone"] = dict(type="FCAF3DBackbone", in_channels=8, depth=34)
    model = build_model(m)
    torch.manual_seed(0)
    model.detection_backbone.init_weights()
    model.detection_head.init_weights()
    return model.to(device).eval()


def test_plugin_keeps_16_bit_maps_on_the_graph_path(device, tmp_path):
    """two detectors with the same weights on six scenes of precomputed channels-last features: one gets fp16 maps and
    static_feature_dtype="keep", the other the same maps widened.  Detections are not compared across the two (the device
    sampler's stream is per detector); the dense volume is"""
    from cnrma_amd import synth
    dims = synth.SHAPES["tiny"][4]
    half = _detector(tmp_path / "half", dims, device, static_feature_dtype="keep")
    full = _detector(tmp_path / "full", dims, device)
    full.load_state_dict(half.state_dict())
    assert half.static_feature_dtype == "keep" and full.static_feature_dtype == "float32"
    names = []
    with torch.no_grad():
        for i in range(6):
            sc = synth.make_scene("tiny", seed=i, boxes=i % 3)
            h = _plant(sc["features"][:, 0], torch.float16, network=True).to(device).contiguous(memory_format=torch.channels_last)
            common = dict(projection=[sc["projection"][:, 0].to(device)], tsdf=sc["tsdf"].to(device),
                          offset=[torch.tensor([0.25 * i, -0.5, 0.125 * (i % 2)], device=device)], scene=[f"scene{i:04d}_00"])
            assert half(return_loss=False, features=[h], **common) == [{}]
            assert full(return_loss=False, features=[h.float()], **common) == [{}]
            names.append(common["scene"][0])
    half.flush()
    full.flush()
    ctx = next(iter(half._static.values()))
    assert ctx["built"] and ctx["k"] == 6 - half.static_calibration
    assert all(st.feature_dtype == torch.float16 for st in ctx["slots"])
    assert all(st.nhwc is None for st in ctx["slots"])                      # nobody allocated a channels-last copy, fp32 or not
    assert all(st.feature_dtype == torch.float32 for st in next(iter(full._static.values()))["slots"])
    assert getattr(half, "static_fallbacks", 0) == 0 and getattr(full, "static_fallbacks", 0) == 0
    assert torch.equal(half.volume, full.volume) and int((half.volume != 0).sum()) > 0
    for d in ("half", "full"):
        for n in names:
            z = np.load(tmp_path / d / "results" / n / f"{n}_bbox_raw.npz")
            assert z["bboxes"].shape[0] == z["scores"].shape[0] > 0
            assert np.isfinite(z["bboxes"]).all() and np.isfinite(z["scores"]).all()
