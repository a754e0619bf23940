"""The 3D U-Net decoder joints on the device (cnrma_amd.unet.join / observed_mask / JointRunner, csrc/unet_join.hip) against the fp64
torch composition of the reference's lines, under the bar of tests/unet_join_cases.py; tests/test_unet_join_cpu.py shows on the same
tensors that the contract in fp32 passes that bar and that each wrong reading of it fails.

Every input is a view inside a NaN-filled allocation (255 for the mask) and `out` is pre-filled with NaN: a read outside a view or a
voxel left unwritten shows.  The fuse kernel's workgroup tile is C.TILE = 4 x 4 x 32 fine voxels."""
import os

import numpy as np
import pytest
import torch

import unet_cases as UC
import unet_fixture as UF
import unet_join_cases as C
from helpers import elementwise_error

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")


def guarded(t, device, guard=4):
    """t as a view `guard` elements into a NaN-filled (uint8: 255-filled) device allocation; guard = 4 floats keeps 16-byte alignment"""
    flat = torch.full((t.numel() + 2 * guard,), 255 if t.dtype == torch.uint8 else NAN, dtype=t.dtype, device=device)
    view = flat[guard:guard + t.numel()].view(t.shape)
    view.copy_(t)
    return view


def run(device, k, step=1, mask=True):
    """-> (out on the host, max of the bound words); the bound's other words must be zero"""
    from cnrma_amd import unet
    d = {n: None if v is None else guarded(v, device) for n, v in k.items()}
    out = torch.full(tuple(k["e"].shape), NAN, device=device)
    y, bound = unet.join(d["xc"], d["e"], d["w_up"], d["w_proj"], d["scale"], d["shift"], observed=d["observed"] if mask else None,
                         step=step, out=out)
    assert y is out and bound.shape == (unet.BOUND_WORDS,)
    words = bound.cpu().view(64, 16)
    assert not words[:, 1:].any() and bool((words[:, 0] >= 0).all())
    return y.cpu(), float(words.max())


def check(label, got, bound, k, step=1, mask=True):
    kk = dict(k, observed=k["observed"] if mask else None)
    ref, mag = C.oracle(**kk, step=step), C.magnitude(**kk, step=step)
    err, bar = C.max_error(got, ref), C.bar(mag, ref)
    print(f"{label}: max|got - ref| {err:.3e}   bar {bar:.3e}   margin {bar / max(err, 1e-300):.1f}   max|ref| {float(ref.abs().max()):.3e}")
    assert got.shape == ref.shape and bool(torch.isfinite(got).all())
    assert err <= bar, (label, err, bar)
    assert bound == float(got.abs().max()), (label, bound, float(got.abs().max()))


@pytest.mark.parametrize("mask", [False, True], ids=["plain", "mask"])
@pytest.mark.parametrize("dims", C.GEOMETRY_DIMS, ids=lambda d: "x".join(map(str, d)))
def test_geometry(device, dims, mask):
    step = 2 if mask else 1
    k = C.make_case(*C.GEOMETRY_WIDTHS, dims, 1, step)
    check(f"geometry {dims}", *run(device, k, step, mask), k, step, mask)


@pytest.mark.parametrize("cc,cf", C.WIDTHS)
def test_widths(device, cc, cf):
    k = C.make_case(cc, cf, C.WIDTH_DIMS)
    check(f"widths {cc} -> {cf}", *run(device, k), k)


@pytest.mark.parametrize("step", C.STEPS)
def test_mask_steps(device, step):
    k = C.make_case(64, 32, (2, 3, 5), 1, step)
    assert 0.3 < float(k["observed"][:, ::step, ::step, ::step].float().mean()) < 0.9
    check(f"step {step}", *run(device, k, step), k, step)


def test_mask_extremes(device):
    step, dims = 2, (3, 3, 17)
    k = C.make_case(64, 32, dims, 1, step)
    plain = run(device, k, mask=False)[0]
    ones = dict(k, observed=torch.ones_like(k["observed"]))
    got, bound = run(device, ones, step)
    check("all observed", got, bound, ones, step)
    assert torch.equal(got, plain)                                               # sel = p everywhere: the maskless result, bit for bit
    none = dict(k, observed=torch.zeros_like(k["observed"]))
    got, bound = run(device, none, step)
    check("none observed", got, bound, none, step)                               # the oracle's where() gives sel = u everywhere
    u = C._conv1(torch.nn.functional.interpolate(k["xc"].double(), scale_factor=2, mode="trilinear", align_corners=False), k["w_up"])
    exp = (u + (u * C._chan(k["scale"], u) + C._chan(k["shift"], u)).relu()) / 2
    assert C.max_error(got, exp) <= C.bar(C.magnitude(**none, step=step), exp)
    last = torch.ones_like(k["observed"])
    X, Y, Z = C.fine(dims)
    last[:, step * (X - 1)] = 0
    last[:, :, step * (Y - 1)] = 0
    last[:, :, :, step * (Z - 1)] = 0
    edge = dict(k, observed=last)
    got, bound = run(device, edge, step)
    check("unobserved at the last index of each axis", got, bound, edge, step)
    assert torch.equal(got[:, :, :-1, :-1, :-1], plain[:, :, :-1, :-1, :-1]) and not torch.equal(got[:, :, -1], plain[:, :, -1])


@pytest.mark.parametrize("case", C.EXACT_CASES, ids=lambda v: str(v).replace(" ", ""))
@pytest.mark.parametrize("mask", [False, True], ids=["plain", "mask"])
def test_exact_inputs_give_the_oracle_bit_for_bit(device, case, mask):
    k = C.exact_case(*case)
    step = case[3]
    got, bound = run(device, k, step, mask)
    ref = C.oracle(**dict(k, observed=k["observed"] if mask else None), step=step)
    assert torch.equal(got.double(), ref) and bound == float(ref.abs().max())


def test_batch_items_do_not_mix(device):
    step, dims = 2, (3, 3, 17)
    k = C.make_case(64, 32, dims, 2, step)
    both, bound = run(device, k, step)
    check("B = 2", both, bound, k, step)
    other = {n: v.clone() if v.dim() > 2 or n == "observed" else v for n, v in k.items()}
    other["xc"][1] += 1.0
    other["e"][1] *= -2.0
    other["observed"][1] = 1 - other["observed"][1]
    changed = run(device, other, step)[0]
    assert torch.equal(changed[0], both[0]) and not torch.equal(changed[1], both[1])
    twice = {n: torch.cat((v[:1], v[:1])) if v.dim() > 2 or n == "observed" else v for n, v in k.items()}
    single = {n: v[:1].contiguous() if v.dim() > 2 or n == "observed" else v for n, v in k.items()}
    got2, got1 = run(device, twice, step)[0], run(device, single, step)[0]
    assert torch.equal(got2[:1], got1) and torch.equal(got2[1:], got1) and torch.equal(got1, both[:1])


def test_zero_scale_and_zero_inputs(device):
    k = C.make_case(64, 32, (2, 3, 5), 1, 2)
    flat = dict(k, scale=torch.zeros(32))
    got, bound = run(device, flat, 2)
    check("scale = 0", got, bound, flat, 2)                                      # out = (u + max(shift, 0)) / 2
    zero = dict(k, xc=torch.zeros_like(k["xc"]), e=torch.zeros_like(k["e"]))
    got, bound = run(device, zero, 2)
    exp = (k["shift"].clamp(min=0) / 2).view(1, -1, 1, 1, 1).expand_as(got)
    assert torch.equal(got, exp) and bound == float(exp.max()) > 0


@pytest.mark.parametrize("peak", ["first", "last", "tail"])
def test_published_bound(device, peak):
    dims = (3, 3, 17)                                                            # fine 6 x 6 x 34: (4, 5, 32) lies in the tail tile of every axis
    k = C.make_case(64, 32, dims)
    at = dict(first=(0, 0, 0), last=(5, 5, 33), tail=(4, 5, 32))[peak]
    e = k["e"].clone()
    e[0, :, at[0], at[1], at[2]] *= 1000.0
    k = dict(k, e=e)
    got, bound = run(device, k, mask=False)
    check(f"peak {peak}", got, bound, k, mask=False)
    where = np.unravel_index(int(got.abs().argmax()), got.shape)
    assert tuple(where[2:]) == at and bound == float(got.abs().max()) > 100


@pytest.mark.parametrize("offset", [4, 5], ids=["aligned", "misaligned"])
@pytest.mark.parametrize("channels", [32, 96])
@pytest.mark.parametrize("dims", [(4, 6, 8), (3, 5, 7), (1, 1, 1), (2, 3, 5)], ids=lambda d: "x".join(map(str, d)))
def test_observed_mask(device, dims, channels, offset):
    from cnrma_amd import unet
    g = torch.Generator().manual_seed(sum(dims) + channels)
    x = torch.randn(2, channels, *dims, generator=g).clamp(-3, 3)
    x = x * (torch.rand(2, channels, *dims, generator=g) < 0.05) * (torch.rand(2, 1, *dims, generator=g) < 0.7)
    x[0, channels // 2, -1, -1, -1] = -3.5
    exp = (x != 0).any(1)
    assert 0 < int(exp.sum()) < exp.numel() or exp.numel() < 4
    observed, bound = unet.observed_mask(guarded(x, device, offset), with_bound=True)
    assert observed.dtype == torch.uint8 and torch.equal(observed.cpu(), exp.to(torch.uint8))
    words = bound.cpu().view(64, 16)
    assert float(words.max()) == float(x.abs().max()) == 3.5 and not words[:, 1:].any()
    assert torch.equal(unet.observed_mask(guarded(x, device, offset)), observed)
    for at in ((0, 0, 0, 0, 0), (1, channels - 1, dims[0] - 1, dims[1] - 1, dims[2] - 1)):
        for value, seen in ((-2.5, 1), (-0.0, 0)):                               # a negative zero stays unobserved
            one = torch.zeros_like(x)
            one[at] = value
            observed, bound = unet.observed_mask(guarded(one, device, offset), with_bound=True)
            assert int(observed.sum()) == seen and int(observed[at[0], at[2], at[3], at[4]]) == seen
            assert float(bound.max()) == abs(value)


def test_two_runs_are_bit_identical(device):
    k = C.make_case(64, 32, (5, 4, 9), 1, 2)
    runs = [run(device, k, 2) for _ in range(2)]
    assert torch.equal(runs[0][0], runs[1][0]) and runs[0][1] == runs[1][1]


def test_refusals_raise_and_launch_nothing(device):
    from cnrma_amd import unet
    from cnrma_amd._lib import CnrmaError
    k = {n: v.to(device) for n, v in C.make_case(64, 32, (2, 3, 5), 1, 2).items()}
    out = torch.full(tuple(k["e"].shape), NAN, device=device)

    def join(**over):
        a = dict(k, step=2, out=out)
        a.update(over)
        return unet.join(a["xc"], a["e"], a["w_up"], a["w_proj"], a["scale"], a["shift"], observed=a["observed"], step=a["step"],
                         out=a["out"])
    with pytest.raises(CnrmaError, match="float32"):
        join(xc=k["xc"].half())
    with pytest.raises(CnrmaError, match="contiguous"):
        join(e=torch.zeros(1, 32, 4, 6, 20, device=device)[..., ::2])
    with pytest.raises(CnrmaError, match="e must be"):                           # e is not exactly twice xc
        join(e=torch.zeros(1, 32, 4, 6, 11, device=device))
    with pytest.raises(CnrmaError, match="e must be"):
        join(e=torch.zeros(2, 32, 4, 6, 10, device=device))
    with pytest.raises(CnrmaError, match="not supported"):
        join(xc=torch.zeros(1, 48, 2, 3, 5, device=device))
    with pytest.raises(CnrmaError, match="w_up must be"):
        join(w_up=k["w_up"].t().contiguous())
    with pytest.raises(CnrmaError, match="w_proj must be"):
        join(w_proj=k["w_proj"][:, :16].contiguous())
    with pytest.raises(CnrmaError, match="scale and shift"):
        join(shift=None)
    with pytest.raises(CnrmaError, match="scale must hold"):
        join(scale=k["scale"][:16])
    with pytest.raises(CnrmaError, match="observed must be"):                    # the mask of another step
        join(step=1)
    with pytest.raises(CnrmaError, match="observed must be"):
        join(observed=k["observed"].float())
    with pytest.raises(CnrmaError, match="step must be"):
        join(step=0)
    with pytest.raises(CnrmaError, match="out must be"):
        join(out=out[:, :, :2])
    with pytest.raises(CnrmaError, match="float32"):
        unet.observed_mask(k["xc"].double())
    with pytest.raises(CnrmaError, match="contiguous"):
        unet.observed_mask(k["e"][..., ::2])
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())


# ---- the whole network
def build(cond, impl, joints="torch", **over):
    import projects.mvsdetection  # noqa: F401
    from projects.mvsdetection.registry import build_backbone
    return build_backbone(dict(type="AtlasBackbone3D", cond_proj=cond, impl=impl, joints=joints, **dict(UF.NET, **over))).eval()


def forbid_torch_joints(monkeypatch):
    """the device joints call neither F.interpolate nor the 1x1x1 modules"""
    def no(*a, **k):
        raise AssertionError("a torch op of the joint ran")
    monkeypatch.setattr(torch.nn.functional, "interpolate", no)


@pytest.mark.parametrize("tag,cond", UF.CASES)
def test_network_matches_the_reference(device, tag, cond, monkeypatch):
    z = np.load(os.path.join(ROOT, "tests", "golden", "atlas3d_wide.npz"))
    x = UF.make_input().to(device)
    net = UF.fill(build(cond, "device", "device")).to(device)
    with torch.no_grad():
        convs_only = UF.fill(build(cond, "device")).to(device)(x)
        forbid_torch_joints(monkeypatch)
        feats = net(x)
    assert net.__dict__["_device_plan"][3] is not None and len(feats) == 2
    for i, (f, fc) in enumerate(zip(feats, convs_only)):
        ref, e32 = z[f"{tag}_feat{i}"], float(z[f"{tag}_fp32_error{i}"])
        err, err_c = elementwise_error(f.cpu().numpy(), ref), elementwise_error(fc.cpu().numpy(), ref)
        print(f"{tag} feat{i}: joints='device' {err:.3e}   joints='torch' {err_c:.3e}   reference fp32 vs its fp64 {e32:.3e}")
        assert f.shape == ref.shape and err <= UC.TOL and err <= 4 * e32, (tag, i, err, e32)


def build_shipped(impl, joints, variant, cond=False):
    import projects.mvsdetection  # noqa: F401
    from projects.mvsdetection.models.backbone3d import BasicBlock3d
    from projects.mvsdetection.registry import build_backbone
    net = UF.fill(build_backbone(dict(UC.shipped_cfg(), impl=impl, joints=joints, cond_proj=cond))).eval().requires_grad_(False)
    if variant == "zeroed":
        for m in [m for m in net.modules() if isinstance(m, BasicBlock3d)][1::2]:
            m.bn2.weight.zero_()
    return net


def check_features(label, got, ref, f32):
    for i, (g, r, f) in enumerate(zip(got, ref, f32)):
        err, e32, bar = UC.max_error(g.cpu(), r), UC.max_error(f, r), UC.net_bar(f, r)
        ew = elementwise_error(g.cpu(), r)
        print(f"{label} feat{i}: device {err:.3e}   fp32 CPU {e32:.3e}   bar {bar:.3e}   elementwise {ew:.3e}")
        assert g.shape == r.shape and bool(torch.isfinite(g).all()) and err <= bar and ew <= UC.TOL, (label, i, err, bar, ew)


@pytest.mark.parametrize("variant", ["filled", "zeroed"])
def test_shipped_network_at_8x8x8(device, variant, monkeypatch):
    ref, f32 = UC.net_reference(variant)
    net = build_shipped("device", "device", variant).to(device)
    forbid_torch_joints(monkeypatch)
    with torch.no_grad():
        got = net(UC.net_input().to(device))
    assert len(got) == 3 and [tuple(g.shape[1:]) for g in got] == [(128, 2, 2, 2), (64, 4, 4, 4), (32, 8, 8, 8)]
    check_features(variant, got, ref, f32)


def test_shipped_network_with_an_unobserved_slab(device):
    x = UC.net_input().clone()
    x[:, :, :3] = 0                                                              # sampled at step 4, 2, 1: coarse x index 0; 0, 1; 0-2
    with torch.no_grad():
        ref = build_shipped("torch", "torch", "filled", cond=True).double()(x.double())
        f32 = build_shipped("torch", "torch", "filled", cond=True)(x)
        plain = build_shipped("torch", "torch", "filled", cond=False)(x)
        got = build_shipped("device", "device", "filled", cond=True).to(device)(x.to(device))
    assert UC.max_error(plain[2], ref[2]) > 1e-2                                 # the condition matters on this input
    check_features("cond", got, ref, f32)


def test_joint_runners_follow_the_weights(device):
    x = UF.make_input()
    net = UF.fill(build(True, "device", "device")).to(device)
    host = UF.fill(build(True, "torch"))
    with torch.no_grad():
        first = [f.cpu() for f in net(x.to(device))]
        plan = net.__dict__["_device_plan"]
        net(x.to(device))
        assert net.__dict__["_device_plan"] is plan                              # unchanged weights: the runners are kept
        for tensor in (lambda m: m.layers_up_conv[0].weight, lambda m: m.proj[0].norm.running_var, lambda m: m.proj[1].conv.weight):
            tensor(net).mul_(1.5)                                                # in place: the version counter moves
            tensor(host).mul_(1.5)
            got, exp = [f.cpu() for f in net(x.to(device))], host(x)
            assert net.__dict__["_device_plan"] is not plan
            plan = net.__dict__["_device_plan"]
            assert all(elementwise_error(a, b) <= UC.TOL for a, b in zip(got, exp))
            assert elementwise_error(first[-1], exp[-1]) > 1e-3                  # the output before the update is no longer right
            first = got
        UF.fill(host, salt="second")
        net.load_state_dict(host.state_dict())
        assert net.__dict__["_device_plan"] is None
        for a, b, c in zip(net(x.to(device)), host(x), first):
            assert elementwise_error(a.cpu(), b) <= UC.TOL and elementwise_error(c, b) > 1e-2


def test_eval_forward_in_a_graph(device):
    """the eval forward with device joints captured once and replayed on other inputs: bit-identical to the eager device result"""
    net = UF.fill(build(True, "device", "device")).to(device)
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
