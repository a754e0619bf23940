"""GPU tests (-m gpu) of the dense 3x3x3 convolutions of the 3D U-Net (csrc/unet.hip, cnrma_amd.unet) and of
AtlasBackbone3D(impl="device").

The oracle is torch.nn.functional.conv3d in fp64 on the CPU with the epilogue composed in fp64.  Every comparison (`check`) holds
two criteria: helpers.elementwise_error <= 1e-4, the project's parity tolerance, on O(1) inputs, and the sparse family's

    max|got - exp| <= 8e-7 * max(sum|a||b| * |scale[c]|) + 4 * 2^-24 * max(1, max|exp|)

(unet_cases.sum_bar; 8e-7 of the largest sum|a||b| is the project's f16x3 figure, established up to this kernel's longest dot,
27 * 256).  The first alone cannot tell f16x3 from an f16x3 that loses a cross term; tests/test_unet_model_cpu.py shows on these
tensors that the second can.  Every case prints the device's figures and those of an fp32 torch convolution next to them before it
asserts, and every device call writes into a y pre-filled with NaN, so an output voxel the kernel skips fails the comparison.
The inputs live in tests/unet_cases.py, shared with that CPU test and with tests/test_unet_edges_gpu.py.

The batch case hands both calls the SAME magnitude bound (that of the two-item tensor, an upper bound of item 0's as well): the
f16x3 split of an element depends on the power-of-two scale once its low half reaches the fp16 subnormals, so bit identity
across calls needs the scale to be the same; with one bound, any difference left would be a halo that crossed a batch item."""
import os

import numpy as np
import pytest
import torch

import unet_cases as C
import unet_fixture as UF
from helpers import elementwise_error
from unet_cases import EDGE_DIMS, TOL, make_case, oracle

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_device(device, x, w, stride=1, scale=None, shift=None, residual=None, relu=False, bound=None, image=None):
    """-> (y on the host, max of the published bound); y was NaN before the call"""
    from cnrma_amd import unet
    image = unet.prepare_conv3_weights(w.to(device)) if image is None else image
    shape = (x.shape[0], w.shape[0], *((n - 1) // stride + 1 for n in x.shape[2:]))
    out = torch.full(shape, float("nan"), device=device)
    mv = lambda t: None if t is None else t.to(device)
    y, bound_y = unet.conv3(x if x.is_cuda else x.to(device), image, stride=stride, scale=mv(scale), shift=mv(shift),
                            residual=mv(residual), relu=relu, bound=bound, out=out)
    assert y is out and bound_y.numel() == unet.BOUND_WORDS
    return y.cpu(), float(bound_y.view(64, 16)[:, 0].max())


def check(label, got, x, w, **kw):
    """the project's parity bound, and the sparse family's criterion beside it: the error against the largest sum|a||b| of the
    comparison (unet_cases.sum_bar; 8e-7 is f16x3's figure), which a lost cross term of the f16x3 product exceeds"""
    ref = oracle(x, w, **kw)
    f32 = oracle(x, w, dtype=torch.float32, **kw)
    err, err32 = elementwise_error(got, ref), elementwise_error(f32, ref)
    print(f"{label}: device {err:.3e}   fp32 torch {err32:.3e}   (criterion {TOL:.0e})")
    assert tuple(got.shape) == tuple(ref.shape) and bool(torch.isfinite(got).all())
    mag = C.magnitude(x, w, **kw)
    top, bar = float(mag.max()), C.sum_bar(mag, ref)
    worst, worst32 = C.max_error(got, ref), C.max_error(f32, ref)
    print(f"{label}: of the largest sum|a||b|: device {worst / top:.3e}   fp32 torch {worst32 / top:.3e}   (bar {bar / top:.3e})")
    assert err <= TOL, (label, err)
    assert worst <= bar, (label, worst, bar)


@pytest.mark.parametrize("dims", EDGE_DIMS, ids=lambda d: "x".join(map(str, d)))
def test_edge_geometry_stride1(device, dims):
    """below one box (8 x 4 x 8 voxels), a box that is full along x and z, partial boxes on every axis, Z no multiple of 4"""
    x, w, _, _ = make_case(32, 32, dims)
    got, _ = run_device(device, x, w)
    check(f"stride 1, 32 -> 32, {dims}", got, x, w)


@pytest.mark.parametrize("cin,cout", C.WIDTHS)
def test_widths(device, cin, cout):
    """one and two channel tiles per wave (Cout % 64), several channel slices per launch, 2 to 16 chunks of input channels"""
    x, w, _, _ = make_case(cin, cout, C.WIDTH_DIMS)
    got, _ = run_device(device, x, w)
    check(f"stride 1, {cin} -> {cout}, (4, 6, 5)", got, x, w)


def test_batch_items_do_not_mix(device):
    from cnrma_amd import unet
    x0, w, _, _ = make_case(32, 64, (5, 7, 9))
    loud = 1e3 * torch.randn(x0.shape, generator=torch.Generator().manual_seed(5))
    x2 = torch.cat((x0, loud)).to(device)
    bound = unet.absmax(x2)
    image = unet.prepare_conv3_weights(w.to(device))
    got2, _ = run_device(device, x2, w, bound=bound, image=image)
    got1, _ = run_device(device, x2[:1], w, bound=bound, image=image)
    assert torch.equal(got2[0], got1[0])                        # bit for bit: no halo of item 0 reaches into item 1
    check("B = 2, item 0 under the common bound", got2[:1], x0, w)
    check("B = 2, item 1 in units of 1e3 (O(1) again)", got2[1:] / 1e3, loud / 1e3, w)
    alone, _ = run_device(device, x0, w, image=image)           # item 0 under its own (1e3 x smaller) bound: within the criterion too
    check("item 0 alone", alone, x0, w)


def test_input_as_a_view_of_a_nan_filled_allocation(device):
    x, w, _, _ = make_case(32, 32, (5, 7, 3))
    big = torch.full((3, *x.shape[1:]), float("nan"), device=device)
    big[1] = x[0].to(device)
    view = big[1:2]
    assert view.is_contiguous() and view.data_ptr() != big.data_ptr()
    got, _ = run_device(device, view, w)
    check("interior view", got, x, w)
    fresh, _ = run_device(device, x, w)
    assert torch.equal(got, fresh)


@pytest.mark.parametrize("cin,cout", C.STRIDE2_WIDTHS)
@pytest.mark.parametrize("dims,odims", C.STRIDE2_DIMS,
                         ids=lambda d: "x".join(map(str, d)))
def test_stride2(device, dims, odims, cin, cout):
    """odd and even sizes (the last tap of an even axis falls outside), one voxel, several boxes"""
    x, w, _, _ = make_case(cin, cout, dims)
    got, _ = run_device(device, x, w, stride=2)
    assert tuple(got.shape[2:]) == odims
    check(f"stride 2, {cin} -> {cout}, {dims}", got, x, w, stride=2)


@pytest.mark.parametrize("mode", C.EPILOGUES)
def test_epilogue(device, mode):
    """undo the scales, * scale + shift, + residual, ReLU -- in that order, against the fp64 composition"""
    x, w, _, _ = make_case(*C.EPILOGUE_SHAPE)
    kw = C.epilogue_kw(mode)
    got, _ = run_device(device, x, w, **kw)
    check(mode, got, x, w, **kw)
    if kw.get("relu"):
        share = float((got == 0).float().mean())
        assert 0.2 < share < 0.8 and float(got.min()) == 0.0    # the ReLU cuts, and it is the last step


def test_power_of_two_scaling_is_exact(device):
    x, w, _, _ = make_case(32, 64, (5, 7, 9))
    base, _ = run_device(device, x, w)
    for p in (10, -10):
        got, _ = run_device(device, x * 2.0 ** p, w)
        assert torch.equal(got, base * 2.0 ** p), p


def test_zero_inputs(device):
    x, w, _, _ = make_case(32, 64, (5, 7, 9))
    got, bound = run_device(device, torch.zeros_like(x), w)
    assert bool((got == 0).all()) and bound == 0.0              # exact zeros, and their bound
    got, bound = run_device(device, x, torch.zeros_like(w))
    assert bool((got == 0).all()) and bound == 0.0
    xz = x.clone()
    xz[:, 5] = 0                                                # one all-zero input channel
    got, _ = run_device(device, xz, w)
    check("channel 5 zero", got, xz, w)


@pytest.mark.parametrize("stride,width", [pytest.param(1, 64, id="1"), pytest.param(2, 64, id="2"), pytest.param(2, 32, id="2-cout32")])
def test_published_bound(device, stride, width):
    """the convention publishes max|y| itself (one atomic maximum per workgroup on its hashed slot): at least max|y|, below
    2 max|y|, and in fact equal to it; a chain of two layers that hands the first bound on equals the chain that recomputes it"""
    from cnrma_amd import unet
    x, w, scale, shift = make_case(width, width, (9, 8, 17))
    got, bound = run_device(device, x, w, stride=stride, scale=scale, shift=shift)
    mx = float(got.abs().max())
    assert mx <= bound < 2 * mx and bound == mx
    image = unet.prepare_conv3_weights(w.to(device))
    y1, b1 = unet.conv3(x.to(device), image, stride=stride)
    handed, _ = unet.conv3(y1, image, bound=b1)
    recomputed, _ = unet.conv3(y1, image)
    assert torch.equal(handed, recomputed)
    assert torch.equal(unet.absmax(y1).view(64, 16)[:, 0].max(), b1.view(64, 16)[:, 0].max())


def test_two_runs_are_bit_identical(device):
    x, w, scale, shift = make_case(64, 64, (9, 8, 17))
    runs = [run_device(device, x, w, scale=scale, shift=shift, residual=x, relu=True) for _ in range(2)]
    assert torch.equal(runs[0][0], runs[1][0]) and runs[0][1] == runs[1][1]


def test_refusals_raise_and_launch_nothing(device):
    from cnrma_amd import unet
    from cnrma_amd._lib import CnrmaError
    x, w, _, _ = make_case(32, 32, (5, 7, 3))
    image = unet.prepare_conv3_weights(w.to(device))
    out = torch.full((1, 32, 5, 7, 3), float("nan"), device=device)
    with pytest.raises(CnrmaError, match="not supported"):                       # Cin = 48 has no image ...
        unet.prepare_conv3_weights(torch.zeros(32, 48, 3, 3, 3, device=device))
    with pytest.raises(CnrmaError, match="48 channels"):                         # ... and no image fits an x of 48 channels
        unet.conv3(torch.zeros(1, 48, 5, 7, 3, device=device), image, out=out)
    with pytest.raises(CnrmaError, match="stride 3"):
        unet.conv3(x.to(device), image, stride=3, out=out)
    wide = torch.zeros(1, 32, 5, 7, 6, device=device)
    with pytest.raises(CnrmaError, match="contiguous"):
        unet.conv3(wide[..., ::2], image, out=out)
    with pytest.raises(CnrmaError, match="contiguous"):
        unet.conv3(torch.zeros(1, 32, 7, 9, 5, device=device)[:, :, 1:-1, 1:-1, 1:-1], image, out=out)
    with pytest.raises(CnrmaError, match="out must be"):
        unet.conv3(x.to(device), image, out=out[:, :, :4])
    with pytest.raises(CnrmaError, match="scale and shift"):
        unet.conv3(x.to(device), image, scale=torch.ones(32, device=device), out=out)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())


def build(cond, impl):
    import projects.mvsdetection  # noqa: F401
    from projects.mvsdetection.registry import build_backbone
    return build_backbone(dict(type="AtlasBackbone3D", cond_proj=cond, impl=impl, **UF.NET)).eval()


@pytest.mark.parametrize("tag,cond", UF.CASES)
def test_network_matches_the_reference(device, tag, cond):
    """the whole module on the device path against the reference's outputs, and the torch path on the same GPU beside it"""
    z = np.load(os.path.join(ROOT, "tests", "golden", "atlas3d_wide.npz"))
    x = UF.make_input().to(device)
    net = UF.fill(build(cond, "device")).to(device)
    with torch.no_grad():
        feats = net(x)
        feats_torch = UF.fill(build(cond, "torch")).to(device)(x)
    assert net.__dict__["_device_plan"] is not None and len(feats) == 2
    for i, (f, ft) in enumerate(zip(feats, feats_torch)):
        ref = z[f"{tag}_feat{i}"]
        err, err_t = elementwise_error(f.cpu().numpy(), ref), elementwise_error(ft.cpu().numpy(), ref)
        print(f"{tag} feat{i}: impl='device' {err:.3e}   impl='torch' on the GPU {err_t:.3e}   reference fp32 vs its fp64 "
              f"{float(z[f'{tag}_fp32_error{i}']):.3e}   (criterion {TOL:.0e})")
        assert f.shape == ref.shape and err <= TOL, (tag, i, err)


def test_weight_images_follow_the_weights(device):
    """load_state_dict, an in-place update and train() each drop the prepared images: the output follows the new weights"""
    x = UF.make_input()
    net = UF.fill(build(True, "device")).to(device)
    host = UF.fill(build(True, "torch"))
    with torch.no_grad():
        first = [f.cpu() for f in net(x.to(device))]
        plan = net.__dict__["_device_plan"]
        net(x.to(device))
        assert net.__dict__["_device_plan"] is plan              # unchanged weights: the images are kept
        UF.fill(host, salt="second")
        net.load_state_dict(host.state_dict())
        assert net.__dict__["_device_plan"] is None
        second = [f.cpu() for f in net(x.to(device))]
        exp = host(x)
        for a, b, c in zip(second, exp, first):
            assert elementwise_error(a, b) <= TOL and elementwise_error(c, b) > 1e-2
        net.layers_down[0][0].conv1.weight.mul_(2.0)             # an optimiser-style in-place step bumps the version counter
        host.layers_down[0][0].conv1.weight.mul_(2.0)
        third = [f.cpu() for f in net(x.to(device))]
        for a, b in zip(third, host(x)):
            assert elementwise_error(a, b) <= TOL
        net.layers_down[0][0].bn1.running_var.data.mul_(4.0)     # through .data: no version bump; train() / eval() drops the images
        host.layers_down[0][0].bn1.running_var.data.mul_(4.0)
        net.train().eval()
        for a, b in zip(net(x.to(device)), host(x)):
            assert elementwise_error(a.cpu(), b) <= TOL


def test_eval_forward_in_a_graph(device):
    """the eval forward captured once and replayed on other inputs: bit-identical to the eager device result"""
    net = UF.fill(build(True, "device")).to(device)
    static_x = UF.make_input().to(device)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), torch.no_grad():
        net(static_x)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph), torch.no_grad():
        out = net(static_x)
    seen = []
    for seed in (3, 20):
        x = UF.make_input().to(device) if seed == 20 else torch.randn(UF.INPUT_SHAPE, generator=torch.Generator().manual_seed(seed)).to(device)
        with torch.no_grad():
            eager = net(x)
        static_x.copy_(x)
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(out, eager):
            assert torch.equal(a, b) and bool(torch.isfinite(a).all())
        seen.append(out[1].clone())
    assert not torch.equal(seen[0], seen[1])
