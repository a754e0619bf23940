"""GPU tests of the device TSDF head (csrc/recon.hip through cnrma_amd.recon and AtlasTSDFHead(impl="device")).

Two kinds of comparison:
  * chains (the fixture from the reference, a mid-size chain, the plugin): every scale sparsifies by its OWN previous output, so a
    parent within 1e-4 (the project's parity tolerance) of the threshold may fall on the other side; the children of such parents
    are excluded and counted, and the count must stay under 1 % of the scale's voxels.  Elsewhere near / far and the fill's sign
    are exact and values and losses agree within 1e-4.
  * one scale on an identical `prev`: nothing is excluded.  Far voxels (fill, sign) and the count of `use` are exact; for values,
    losses and gradients the device's error against the float64 oracle (tests/recon_oracle.py) must not exceed
    max(4 x the error of the torch module's float32 arithmetic against the same oracle, 1e-6 max|ref|) -- the rule of
    tests/test_sparse_backward_edges_gpu.py.  Every figure is printed before it is asserted."""
import os

import numpy as np
import pytest
import torch

import recon_oracle as RO

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("016", "008", "004")
LS, THR = 1.05, 0.99
TOL, MARGIN, CAP = 1e-4, 1e-4, 0.01


# ---- inputs ---------------------------------------------------------------------------------------------------------------------

def make_scale(seed, B, C, dims, first=False, w_std=None, prev_kind="mixed"):
    """x [B,C,*dims], w [C], prev [B,1,*dims/2] (None at a first scale), target [B,1,*dims]: CPU tensors fixed by the seed.
    prev mixes regressed values on both sides of the threshold with the fill values +-0.999 and zeros; the target holds observed
    values, unobserved ones (exactly 1) inside observed columns and an x-slab of fully empty columns"""
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(B, C, *dims, generator=gen)
    w = torch.randn(C, generator=gen) * (w_std if w_std is not None else 1.0 / C ** 0.5)
    prev = None
    if not first:
        half = tuple(n // 2 for n in dims)
        prev = (torch.randn(B, 1, *half, generator=gen) * 0.9).clamp(-LS, LS)
        pick = torch.rand(B, 1, *half, generator=gen)
        prev[pick < 0.15] = 0.999
        prev[pick < 0.08] = -0.999
        prev[pick > 0.97] = 0.0
        if prev_kind == "far":
            prev = torch.where(prev < 0, -1.0, 1.0) * (0.99 + 0.06 * torch.rand(B, 1, *half, generator=gen))
        elif prev_kind == "near":
            prev = prev.clamp(-0.98, 0.98)
    target = torch.rand(B, 1, *dims, generator=gen) * 2 - 1
    target[torch.rand(B, 1, *dims, generator=gen) < 0.2] = 1.0
    target[:, :, : max(1, dims[0] // 4)] = 1.0
    return x, w, prev, target


def bar_ok(label, got, tor, ref):
    """device error <= max(4 x torch error, 1e-6 max|ref|), printed first"""
    got, tor, ref = (torch.as_tensor(t).detach().double().cpu() for t in (got, tor, ref))
    if ref.numel() == 0:
        return True
    finite = torch.isfinite(ref)
    assert torch.equal(torch.isnan(got), torch.isnan(ref)), label
    e_k = float((got - ref)[finite].abs().max()) if finite.any() else 0.0
    e_t = float((tor - ref)[finite].abs().max()) if finite.any() else 0.0
    scale = float(ref[finite].abs().max()) if finite.any() else 0.0
    bar = max(4 * e_t, 1e-6 * scale)
    print("%-28s device %.3e torch %.3e max|ref| %.3e bar %.3e" % (label, e_k, e_t, scale, bar))
    return e_k <= bar


def run_device(x, w, prev, target, threshold=THR, grad_tsdf=None, grad_loss=1.7):
    """-> dict(tsdf, loss, count, dx, dw) of the device scale; the gradients of grad_loss * loss (+ sum(tsdf * grad_tsdf))"""
    from cnrma_amd import recon
    x = x.detach().clone().requires_grad_(True)
    w = w.detach().clone().requires_grad_(True)
    prevg = None if prev is None else prev.detach().clone().requires_grad_(True)
    tsdf, loss, count = recon.tsdf_head_scale(x, w, prevg, threshold, LS, target, return_count=True)
    res = dict(tsdf=tsdf.detach(), loss=None if loss is None else loss.detach(), count=count, dx=None, dw=None)
    total = None
    if loss is not None and grad_loss is not None:
        total = loss * grad_loss
    if grad_tsdf is not None:
        total = (tsdf * grad_tsdf).sum() + (0 if total is None else total)
    if total is not None:
        total.backward()
        res.update(dx=x.grad, dw=w.grad)
        assert prevg is None or prevg.grad is None or not bool(prevg.grad.any())          # prev receives no gradient
    return res


def run_oracle(x, w, prev, target, dtype, threshold=THR, grad_tsdf=None, grad_loss=1.7):
    x = x.detach().to(dtype).requires_grad_(True)
    w = w.detach().to(dtype).requires_grad_(True)
    r = RO.scale(x, w, prev, threshold, LS, target, dtype=dtype)
    total = None
    if r["loss"] is not None and grad_loss is not None:
        total = r["loss"] * grad_loss
    if grad_tsdf is not None:
        total = (r["tsdf"] * grad_tsdf.to(dtype)).sum() + (0 if total is None else total)
    if total is not None:
        total.backward()
        r.update(dx=x.grad, dw=w.grad)
    r["tsdf"] = r["tsdf"].detach()
    r["loss"] = None if r["loss"] is None else r["loss"].detach()
    return r


def check_scale(device, label, x, w, prev, target, threshold=THR, with_grad_tsdf=(False, True)):
    """forward + loss + both backward modes of one scale on an identical prev against the oracle and the torch arithmetic"""
    x, w, target = x.to(device), w.to(device), target.to(device)
    prev = None if prev is None else prev.to(device)
    gen = torch.Generator().manual_seed(1)
    G = torch.randn(target.shape, generator=gen).to(device)
    bad = []
    for mode in with_grad_tsdf:
        g = G if mode else None
        dev = run_device(x, w, prev, target, threshold, g)
        ref = run_oracle(x, w, prev, target, torch.float64, threshold, g)
        tor = run_oracle(x, w, prev, target, torch.float32, threshold, g)
        far = ~ref["near"]
        assert torch.equal(dev["tsdf"][far], ref["tsdf"][far].float()), label           # near / far and the fill's sign: exact
        assert int(dev["count"]) == ref["count"], (label, int(dev["count"]), ref["count"])
        if ref["count"] == 0:
            assert (torch.isnan(dev["loss"]) if prev is None else float(dev["loss"]) == 0.0), (label, dev["loss"])
        for name in ("tsdf", "loss", "dx", "dw"):
            if not bar_ok(f"{label} g{int(mode)} {name}", dev[name], tor[name], ref[name]):
                bad.append((mode, name))
        assert dev["dx"].dtype == x.dtype and dev["dw"].shape == w.shape
        assert not bool((dev["dx"] * far).any())                                        # no gradient where the voxel is filled
    assert not bad, (label, bad)
    return dev


# ---- fixture chain ----------------------------------------------------------------------------------------------------------------

def load_case(name):
    z = np.load(os.path.join(ROOT, "tests", "golden", "tsdf_head.npz"))
    pick = lambda what: [torch.from_numpy(z[f"{name}_{what}{i}"]) for i in range(3)]
    return dict(xs=pick("x"), ws=pick("w"), targets=pick("gt"), tsdfs=pick("tsdf"), losses=pick("loss"),
                label_smoothing=float(z["label_smoothing"]), thresholds=[float(t) for t in z["thresholds"]])


def build_head(channels, ws, impl, thresholds=(THR, THR, THR), ls=LS):
    import projects.mvsdetection  # noqa: F401
    from projects.mvsdetection.registry import build_head as build
    head = build(dict(type="AtlasTSDFHead", input_channels=list(channels)[::-1], n_scales=len(channels), voxel_size=0.04,
                      label_smoothing=ls, sparse_threshold=list(thresholds), impl=impl))
    for dec, w in zip(head.decoders, ws):
        dec.weight.data.copy_(w.reshape(dec.weight.shape))
    return head


def compare_chain(label, got_tsdfs, got_losses, ref_tsdfs, ref_losses, thresholds, counts=None):
    """a chain against a reference chain: children of parents within MARGIN of the threshold (on either side's parent) are
    excluded and counted (cap 1 %); elsewhere the fill is exact and values within TOL; losses within TOL (an excluded voxel can
    move a mean over `count` voxels by at most 2 log(2.05) / count)"""
    for i, (got, ref) in enumerate(zip(got_tsdfs, ref_tsdfs)):
        got, ref = got.detach().cpu(), ref.detach().cpu().float()
        keep = torch.ones_like(ref, dtype=torch.bool)
        if i:
            for parent in (got_tsdfs[i - 1], ref_tsdfs[i - 1]):
                up = RO.upsample(parent.detach().cpu().float())
                keep &= (up.abs() - thresholds[i - 1]).abs() > MARGIN
            far = ~(RO.upsample(ref_tsdfs[i - 1].detach().cpu().float()).abs() < thresholds[i - 1])
            assert torch.equal(got[far & keep], ref[far & keep]), (label, i)
        excluded = int((~keep).sum())
        err = float((got - ref)[keep].abs().max()) if keep.any() else 0.0
        print(f"{label} scale {i}: excluded {excluded} of {keep.numel()}, max |tsdf - ref| {err:.3e}")
        assert excluded < CAP * keep.numel() and err <= TOL, (label, i, excluded, err)
        if got_losses is not None:
            gl, rl = float(got_losses[i]), float(ref_losses[i])
            print(f"{label} scale {i}: loss {gl!r} ref {rl!r}")
            if np.isnan(rl):
                assert np.isnan(gl)
            elif rl == 0.0 and excluded == 0:
                assert gl == 0.0 and not np.signbit(gl)
            else:
                slack = 0.0 if excluded == 0 else excluded * 2 * np.log(2.05) / max(1, (counts or {}).get(i, 1))
                assert abs(gl - rl) <= TOL + slack, (label, i, gl, rl)


@pytest.mark.parametrize("name", ["mixed", "allfar", "allnear", "empty0"])
def test_fixture_chain_matches_the_reference(device, name):
    c = load_case(name)
    head = build_head([x.shape[1] for x in c["xs"]], c["ws"], "device", c["thresholds"], c["label_smoothing"]).to(device)
    with torch.no_grad():
        out, losses = head([x.to(device) for x in c["xs"]], {"tsdf_gt_" + k: t.to(device) for k, t in zip(KEYS, c["targets"])})
    assert list(out) == ["scene_tsdf_" + k for k in KEYS] and list(losses) == ["tsdf_loss_" + k for k in KEYS]
    assert all(v.is_cuda and v.dim() == 0 and v.dtype == torch.float32 for v in losses.values())       # device scalars
    compare_chain(name, [out["scene_tsdf_" + k] for k in KEYS], [losses["tsdf_loss_" + k] for k in KEYS], c["tsdfs"], c["losses"],
                  c["thresholds"])


# ---- one scale, identical prev ----------------------------------------------------------------------------------------------------

EDGE = [  # label, B, C, dims, first
    ("2x2x2", 1, 1, (2, 2, 2), False),
    ("z2", 1, 2, (4, 6, 2), False),
    ("z6", 1, 3, (4, 4, 6), False),
    ("z10", 2, 5, (2, 6, 10), False),
    ("ragged", 2, 5, (10, 6, 14), False),
    ("c32", 1, 32, (6, 4, 10), False),
    ("first-odd", 2, 3, (3, 5, 7), True),
    ("mid", 1, 32, (48, 48, 20), False),
]


@pytest.mark.parametrize("label,B,C,dims,first", EDGE, ids=[e[0] for e in EDGE])
def test_scale_matches_oracle_at_edge_shapes(device, label, B, C, dims, first):
    x, w, prev, target = make_scale(100 + len(label) + C, B, C, dims, first)
    dev = check_scale(device, label, x, w, prev, target)
    if not first:
        near = RO.near_mask(prev, THR)
        assert 0 < int(near.sum()) < near.numel() or near.numel() <= 8
    assert int(dev["count"]) > 0


def test_all_far_and_all_near_scales(device):
    x, w, prev, target = make_scale(7, 2, 3, (4, 6, 6), prev_kind="far")
    assert not bool(RO.near_mask(prev, THR).any())
    dev = check_scale(device, "all-far", x, w, prev, target)
    assert int(dev["count"]) == 0 and float(dev["loss"]) == 0.0 and not np.signbit(float(dev["loss"]))
    assert not bool(dev["dx"].any()) and not bool(dev["dw"].any())
    assert bool((dev["tsdf"].abs() == np.float32(0.999)).all()) and {float(s) for s in dev["tsdf"].sign().unique()} == {-1.0, 1.0}
    x, w, prev, target = make_scale(8, 2, 3, (4, 6, 6), prev_kind="near")
    assert bool(RO.near_mask(prev, THR).all())
    check_scale(device, "all-near", x, w, prev, target)


def test_empty_use(device):
    """no usable target voxel: NaN at the first scale (the mean of nothing), exactly 0.0 later; no gradient either way"""
    for first in (True, False):
        x, w, prev, target = make_scale(9, 1, 3, (4, 4, 6), first)
        target = torch.ones_like(target)
        target[..., 0] = 1.5                                  # nothing observed, no column all ones
        dev = check_scale(device, f"empty first={first}", x, w, prev, target, with_grad_tsdf=(False,))
        assert int(dev["count"]) == 0 and (torch.isnan(dev["loss"]) if first else float(dev["loss"]) == 0.0)
        assert not bool(dev["dx"].any()) and not bool(dev["dw"].any())


def test_zero_weights_target_equal_prediction_and_nan_parent(device):
    from cnrma_amd import recon
    # zero weights: tsdf == 0 on every near voxel, where d lt / d tsdf is taken as 0: no loss gradient
    x, w, prev, target = make_scale(10, 1, 5, (4, 6, 6))
    dev = check_scale(device, "zero-w", x, torch.zeros_like(w), prev, target, with_grad_tsdf=(False,))
    near = RO.near_mask(prev, THR).to(device)
    assert not bool(dev["tsdf"][near].any()) and not bool(dev["dx"].any()) and not bool(dev["dw"].any())
    # a target equal to the prediction: zero loss, zero gradient (the sign of nothing is 0)
    xd, wd, pd = x.to(device), w.to(device), prev.to(device)
    pred = recon.tsdf_head_scale(xd, wd, pd, THR, LS)[0]
    dev = run_device(xd, wd, pd, pred.clone())
    assert float(dev["loss"]) == 0.0 and int(dev["count"]) > 0 and not bool(dev["dx"].any()) and not bool(dev["dw"].any())
    tor = run_oracle(xd, wd, pd, RO.scale(xd, wd, pd, THR, LS, dtype=torch.float32)["tsdf"].detach(), torch.float32)
    assert float(tor["loss"]) == 0.0 and not bool(tor["dx"].any())                       # as the torch arithmetic has it
    # a NaN parent is not near: its children are filled with sign(NaN) * 0.999 = 0 and take no part in the loss
    prev_nan = prev.clone()
    prev_nan[0, 0, 1, 1, 1] = float("nan")
    dev = check_scale(device, "nan-parent", x, w, prev_nan, target)
    assert not bool(dev["tsdf"][0, 0, 2:4, 2:4, 2:4].any()) and bool(torch.isfinite(dev["tsdf"]).all())


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_sixteen_bit_inputs_are_read_in_place_bit_for_bit(device, dtype):
    """outputs, losses and dw equal the fp32 kernel's on x.float() bit for bit; dx comes back in x's dtype, rounded once"""
    for label, B, C, dims, first in (EDGE[4], EDGE[6], EDGE[7]):
        x, w, prev, target = make_scale(11, B, C, dims, first)
        x16 = x.to(dtype).to(device)
        args = (w.to(device), None if prev is None else prev.to(device), target.to(device))
        G = torch.randn(target.shape, generator=torch.Generator().manual_seed(2)).to(device)
        lo = run_device(x16, *args, grad_tsdf=G)
        hi = run_device(x16.float(), *args, grad_tsdf=G)
        assert torch.equal(lo["tsdf"], hi["tsdf"]) and torch.equal(lo["loss"], hi["loss"]) and torch.equal(lo["count"], hi["count"])
        assert lo["dx"].dtype == dtype and hi["dx"].dtype == torch.float32
        assert torch.equal(lo["dx"], hi["dx"].to(dtype)) and torch.equal(lo["dw"], hi["dw"])
        assert bool(lo["dx"].any())
    head = build_head([4, 8], [torch.randn(4), torch.randn(8)], "device", (THR,)).to(device)
    xs = [torch.randn(1, 4, 2, 2, 2, device=device, dtype=dtype), torch.randn(1, 8, 4, 4, 4, device=device, dtype=dtype)]
    out, _ = head(xs)                                          # the module hands 16-bit volumes over as they are
    ref, _ = head([x.float() for x in xs])
    assert all(torch.equal(out[k], ref[k]) and out[k].dtype == torch.float32 for k in out)


def test_two_runs_are_bit_identical(device):
    x, w, prev, target = make_scale(12, 1, 32, (48, 48, 20))
    args = (x.to(device), w.to(device), prev.to(device), target.to(device))
    G = torch.randn(target.shape, generator=torch.Generator().manual_seed(3)).to(device)
    a, b = run_device(*args, grad_tsdf=G), run_device(*args, grad_tsdf=G)
    for name in ("tsdf", "loss", "count", "dx", "dw"):
        assert torch.equal(a[name], b[name]), name
    assert bool(torch.isfinite(a["loss"])) and bool(a["dw"].any())


def test_mid_size_chain(device):
    """(12,12,5) -> (24,24,10) -> (48,48,20), C = 8 / 16 / 32: several workgroups and both reduction stages, against the
    float64 chain"""
    gen = torch.Generator().manual_seed(13)
    dims = [(12, 12, 5), (24, 24, 10), (48, 48, 20)]
    channels = (8, 16, 32)
    xs = [torch.randn(1, c, *d, generator=gen) for c, d in zip(channels, dims)]
    ws = [torch.randn(c, generator=gen) * 1.2 / c ** 0.5 for c in channels]
    targets = [make_scale(14 + i, 1, 1, d, True)[3] for i, d in enumerate(dims)]
    head = build_head(channels, ws, "device").to(device)
    with torch.no_grad():
        out, losses = head([x.to(device) for x in xs], {"tsdf_gt_" + k: t.to(device) for k, t in zip(KEYS, targets)})
    ref = RO.chain([x.to(device) for x in xs], [w.to(device) for w in ws], [THR] * 3, LS, [t.to(device) for t in targets])
    far = [float((~r["near"]).float().mean()) for r in ref]
    print("far share", far)
    assert 0.02 < far[1] < 0.98 and 0.02 < far[2] < 0.98
    compare_chain("mid", [out["scene_tsdf_" + k] for k in KEYS], [losses["tsdf_loss_" + k] for k in KEYS],
                  [r["tsdf"] for r in ref], [r["loss"] for r in ref], [THR] * 3, {i: r["count"] for i, r in enumerate(ref)})


def test_forward_and_loss_in_a_graph(device):
    """all three scales with their losses captured once on a side stream, replayed on other inputs of the same shape: the replay
    equals the eager device result bit for bit (nothing in the calls reads the device or synchronises)"""
    from cnrma_amd import recon
    dims = [(3, 3, 2), (6, 6, 4), (12, 12, 8)]
    channels = (3, 5, 8)

    def inputs(seed):
        gen = torch.Generator().manual_seed(seed)
        xs = [torch.randn(2, c, *d, generator=gen).to(device) for c, d in zip(channels, dims)]
        targets = {"tsdf_gt_" + k: make_scale(seed + i, 2, 1, d, True)[3].to(device) for i, (k, d) in enumerate(zip(KEYS, dims))}
        return xs, targets
    ws = [(torch.randn(c, generator=torch.Generator().manual_seed(c)) * 1.5).to(device) for c in channels]
    run = lambda xs, targets: recon.tsdf_head(xs, ws, [THR] * 3, LS, targets)
    static_xs, static_targets = inputs(20)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), torch.no_grad():
        run(static_xs, static_targets)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph), torch.no_grad():
        out, losses = run(static_xs, static_targets)
    replayed = {}
    for seed in (21, 20):
        xs, targets = inputs(seed)
        with torch.no_grad():
            e_out, e_losses = run(xs, targets)
        for s, x in zip(static_xs, xs):
            s.copy_(x)
        for k in targets:
            static_targets[k].copy_(targets[k])
        graph.replay()
        torch.cuda.synchronize()
        for k in e_out:
            assert torch.equal(out[k], e_out[k]), k
        for k in e_losses:
            assert torch.equal(losses[k], e_losses[k]) and bool(torch.isfinite(losses[k])), k
        replayed[seed] = (out["scene_tsdf_004"].clone(), losses["tsdf_loss_004"].clone())
    assert not torch.equal(replayed[20][0], replayed[21][0]) and not torch.equal(replayed[20][1], replayed[21][1])


def test_rejections_raise_and_launch_nothing(device):
    from cnrma_amd import _lib, recon
    from cnrma_amd._lib import CnrmaError, ptr
    x = torch.randn(1, 3, 4, 6, 6, device=device)
    w = torch.randn(3, device=device)
    with pytest.raises(CnrmaError, match="invalid argument"):
        recon.tsdf_head_scale(x, w, torch.zeros(1, 1, 2, 3, 2, device=device), THR, LS)              # not twice prev's
    with pytest.raises(CnrmaError, match="invalid argument"):
        recon.tsdf_head_scale(x, w, torch.zeros(1, 1, 4, 6, 6, device=device), THR, LS)
    with pytest.raises(CnrmaError, match="contiguous"):
        recon.tsdf_head_scale(x.transpose(2, 3), w, None, THR, LS)
    with pytest.raises(CnrmaError, match="float64"):
        recon.tsdf_head_scale(x.double(), w, None, THR, LS)
    with pytest.raises(CnrmaError, match="GPU"):
        recon.tsdf_head_scale(x.cpu(), w.cpu(), None, THR, LS)
    # the entry point itself: -EINVAL, and the output buffer is untouched
    out = torch.full((1, 1, 4, 6, 6), 7.0, device=device)
    prev = torch.zeros(1, 1, 2, 3, 2, device=device)
    for bad in (dict(pz=2), dict(elem=3), dict(X=5)):
        a = dict(dict(elem=0, pz=3, X=4), **bad)
        with pytest.raises(CnrmaError, match="invalid argument"):
            _lib.call_recon("cnrma_recon_head_forward", ptr(x), a["elem"], ptr(w), ptr(prev), 2, 3, a["pz"], THR, LS, 1, 3, a["X"],
                            6, 6, ptr(out), _lib.stream())
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())


# ---- plugin -----------------------------------------------------------------------------------------------------------------------

def test_plugin_with_device_head(device, tmp_path):
    """RayMarching from the shipped config's model section (its 3D U-Net and three-scale head, tsdf_head.impl='device') at the
    smallest grid near the fixtures' that the U-Net accepts (every axis a multiple of 8; the 2D network is left out and the sparse
    detector shrunk to depth 14 as in tests/test_plugin_gpu.py): forward_test and a train_step run, and on the same decoder
    features the head's outputs and losses match impl='torch' under the per-scale rule"""
    import runpy
    import projects.mvsdetection  # noqa: F401
    from projects.mvsdetection.registry import build_model
    from cnrma_amd import synth
    dims = (48, 48, 24)
    sc = synth.make_scene((3, 32, 30, 40, dims, 4), seed=5)
    cfg = runpy.run_path(os.path.join(ROOT, "projects", "configs", "mvsdetection", "ray_marching_scannet.py"))

    def build(impl):
        m = dict(cfg["model"])
        assert m["tsdf_head"]["type"] == "AtlasTSDFHead" and "impl" not in m["tsdf_head"]         # the shipped configs are not edited
        m.update(backbone2d=None, feature_2d=None, save_path=str(tmp_path / impl), voxel_dim_test=list(dims),
                 voxel_dim_train=list(dims), max_points=None, use_feature_transform=False,
                 detection_backbone=dict(type="FCAF3DBackbone", in_channels=32, depth=14),
                 tsdf_head=dict(m["tsdf_head"], impl=impl))
        torch.manual_seed(4)
        model = build_model(m)
        model.detection_backbone.init_weights()
        model.detection_head.init_weights()
        return model.to(device)
    model, twin = build("device"), build("torch")
    with torch.no_grad():                                      # zero_init_residual leaves the decoders' inputs tame: spread them
        for dec in model.tsdf_head.decoders:
            dec.weight.mul_(6.0)
    twin.load_state_dict(model.state_dict())
    assert model.tsdf_head.impl == "device" and twin.tsdf_head.impl == "torch"
    feats = sc["features"][:, 0].to(device).requires_grad_(True)
    gt = sc["tsdf"].to(device).clamp(-1, 1)
    pool = torch.nn.functional.avg_pool3d
    tsdf_list = {"tsdf_gt_004": gt, "tsdf_gt_008": pool(gt, 2), "tsdf_gt_016": pool(gt, 4)}
    data = dict(features=[feats], projection=[sc["projection"][:, 0].to(device)], offset=[torch.zeros(3, device=device)])
    model.eval()
    with torch.no_grad():
        assert model(return_loss=False, scene=["s"], **data) == [{}]
        decoded = [f.contiguous() for f in model.backbone3d(model.volume)]
        out_d, loss_d = model.tsdf_head(decoded, tsdf_list)
        out_t, loss_t = twin.tsdf_head(decoded, tsdf_list)
    assert list(out_d) == list(out_t) and list(loss_d) == list(loss_t) == ["tsdf_loss_" + k for k in KEYS]
    ws = [dec.weight.detach().reshape(-1) for dec in model.tsdf_head.decoders]
    ref = RO.chain(decoded, ws, [THR] * 3, LS, [tsdf_list["tsdf_gt_" + k] for k in KEYS])
    bad = []
    for i, k in enumerate(KEYS):
        keep = torch.ones_like(ref[i]["near"])
        if i:
            for parent in (out_d["scene_tsdf_" + KEYS[i - 1]], out_t["scene_tsdf_" + KEYS[i - 1]], ref[i - 1]["tsdf"].float()):
                keep &= (RO.upsample(parent).abs() - THR).abs() > MARGIN
        excluded = int((~keep).sum())
        print(f"plugin scale {k}: excluded {excluded} of {keep.numel()}, far {float((~ref[i]['near']).float().mean()):.3f}")
        assert excluded < CAP * keep.numel()
        pick = lambda t: t.double()[keep]
        if not bar_ok(f"plugin scene_tsdf_{k}", pick(out_d["scene_tsdf_" + k]), pick(out_t["scene_tsdf_" + k]), pick(ref[i]["tsdf"])):
            bad.append(k)
        if excluded == 0 and not bar_ok(f"plugin tsdf_loss_{k}", loss_d["tsdf_loss_" + k], loss_t["tsdf_loss_" + k], ref[i]["loss"]):
            bad.append("loss " + k)
    assert not bad, bad
    model.train()
    out = model.train_step(dict(data, gt_bboxes_3d=[torch.tensor([[1.0, 1.0, 0.2, 0.6, 0.5, 0.5, 0.0]], device=device)],
                                gt_labels_3d=[torch.tensor([2], device=device)], tsdf_list=tsdf_list), None)
    assert {"tsdf_loss_004", "tsdf_loss_008", "tsdf_loss_016", "loss_cls"} <= set(out["log_vars"])
    out["loss"].backward()
    assert torch.isfinite(out["loss"]) and torch.isfinite(feats.grad).all() and float(feats.grad.abs().sum()) > 0
    grads = [dec.weight.grad for dec in model.tsdf_head.decoders]
    assert all(g is not None and torch.isfinite(g).all() and bool(g.any()) for g in grads)
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in model.backbone3d.parameters())
