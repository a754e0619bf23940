"""GPU tests (-m gpu) of csrc/unet.hip at the places its first suite could not see: f16x3 accuracy itself, the fourth kernel form,
the magnitude-bound pass at every alignment and size, and the shipped architecture.

* Exactness: inputs on which f16x3 has nothing to round (unet_cases.exact_case states why), compared with torch.equal.  Every
  output is one product at a shifted voxel, so every tap direction, every zero halo and the epilogue's register-to-channel map are
  checked bit for bit, and a lost cross term changes the low bits of every output.
* Scales 2^100 apart: the unscaling and f16_scale_for across the exponent range.
* launch_conv3<2, 1, 1, 2> (stride 2, Cout no multiple of 64), under the sum|a||b| bar of test_unet_gpu.check.
* A wide dynamic range: a voxel 2^12 above the rest sets the scale; the quiet outputs are held to 8e-7 of their OWN sum|a||b|.
* unet.absmax against x.abs().max(): sizes around the vector width, a second trip of the grid-stride loop, views 0 to 3 floats
  off 16-byte alignment inside an allocation whose other elements are larger than the view's maximum.
* backbone_3d_cfg() with impl="device" at 8 x 8 x 8 (levels of 8, 4, 2 and 1 voxels; 256 channels; bounds handed through up to
  four blocks of a level; a folded scale of exactly 0) against the same module in fp64 on the CPU.

tests/test_unet_model_cpu.py establishes on the same tensors (tests/unet_cases.py) that the ideal arithmetic and an fp32 torch
convolution pass each of these bars, and that an f16x3 with a lost cross term does not."""
import pytest
import torch

import unet_cases as C
from helpers import elementwise_error
from test_unet_gpu import check, run_device

pytestmark = pytest.mark.gpu

IDS = lambda v: str(v).replace(" ", "")


@pytest.mark.parametrize("kind,widths,dims,stride", C.EXACT_CASES, ids=IDS)
def test_exact_inputs_are_reproduced_bit_for_bit(device, kind, widths, dims, stride):
    """strides 1 and 2; 32 -> 32, 64 -> 64 and 64 -> 96: one and two channel tiles per wave, several channel slices; (9, 6, 11): two
    boxes along x at stride 1, partial boxes on every axis, odd sizes under stride 2; (1, 1, 1): only the centre tap is inside"""
    x, w = C.exact_case(kind, *widths, dims)
    exp = C.oracle(x, w, stride=stride).float()
    got, bound = run_device(device, x, w, stride=stride)
    wrong = int((got != exp).sum())
    print(f"{kind} {widths} {dims} stride {stride}: {wrong} of {exp.numel()} outputs differ, {int((exp != 0).sum())} are nonzero")
    assert torch.equal(got, exp)
    assert bound == float(exp.abs().max())


@pytest.mark.parametrize("px,pw", C.FAR_SCALES)
def test_scales_far_apart_are_undone_exactly(device, px, pw):
    """x * 2^60 with w * 2^40, and x * 2^-40 with w * 2^-30: the same fp16 planes under scales 2^100 and 2^70 away, so the result is
    the base result times that power of two, bit for bit; every output stays a normal fp32 number"""
    x, w, _, _ = C.make_case(*C.FAR_SHAPE)
    base, _ = run_device(device, x, w)
    exp = base * 2.0 ** (px + pw)
    assert float(exp.abs()[exp != 0].min()) >= 2.0 ** -126 and bool(torch.isfinite(exp).all())
    got, bound = run_device(device, x * 2.0 ** px, w * 2.0 ** pw)
    assert torch.equal(got, exp), (px, pw)
    assert bound == float(exp.abs().max())


@pytest.mark.parametrize("dims", C.NARROW_STRIDE2_DIMS, ids=IDS)
@pytest.mark.parametrize("cin,cout", C.NARROW_STRIDE2_WIDTHS)
def test_stride2_narrow_cout(device, cin, cout, dims):
    """launch_conv3<2, 1, 1, 2>: one channel tile per wave under stride 2 (a stem to 32, 96, 160 or 224 channels).  One voxel, odd and
    even sizes, Z over two boxes, and (7, 3, 3): two boxes along x"""
    x, w, _, _ = C.make_case(cin, cout, dims)
    got, _ = run_device(device, x, w, stride=2)
    assert tuple(got.shape[2:]) == tuple((n + 1) // 2 for n in dims)
    check(f"stride 2, {cin} -> {cout}, {dims}", got, x, w, stride=2)


def test_wide_dynamic_range(device):
    """f16x3.h: every element down to 2^-17 of the largest keeps 22 bits.  Here the largest is 2^12 above the rest, and each quiet
    output is held to 8e-7 of its own sum|a||b| (plus four roundings of itself).  The ideal arithmetic keeps a margin of 45 to that
    bar and an fp32 torch convolution one of 10 (tests/test_unet_model_cpu.py); the outputs next to the loud voxel are under the
    usual bar"""
    x, w, quiet = C.wide_case()
    got, _ = run_device(device, x, w)
    ref, mag = C.oracle(x, w), C.magnitude(x, w)
    margin = C.wide_margin(got, ref, mag, quiet)
    margin32 = C.wide_margin(C.oracle(x, w, dtype=torch.float32), ref, mag, quiet)
    px, pw, _, _ = C.make_case(*C.WIDE_SHAPE)                     # the same tensors without the loud voxel, for the record
    plain = C.wide_margin(run_device(device, px, pw)[0], C.oracle(px, pw), C.magnitude(px, pw), torch.ones_like(quiet))
    print(f"wide range: margin to the per-element bar: device {margin:.2f}   fp32 torch {margin32:.2f}   "
          f"(device without the loud voxel, over all outputs: {plain:.2f})")
    assert margin >= 1.0, margin
    assert plain >= 1.0, plain
    check("wide range, all outputs", got, x, w)


@pytest.mark.parametrize("n", C.ABSMAX_SIZES)
def test_absmax_is_exact_and_stays_inside_its_view(device, n):
    """the vector path (offset 0), the scalar path (offsets 1 to 3), the tail and, at the largest n, the grid-stride loop's second
    trip; the peak first, last, in the middle and at the start of the last group of four, positive and negative"""
    from cnrma_amd import unet
    for offset in C.ABSMAX_OFFSETS:
        for peak in C.ABSMAX_PEAKS if n else C.ABSMAX_PEAKS[:1]:
            alloc, start, exp = C.absmax_case(n, offset, peak)
            view = alloc.to(device)[start:start + n]
            assert view.is_contiguous() and (n == 0 or view.data_ptr() % 16 == 4 * offset)
            bound = unet.absmax(view)
            slots = bound.view(64, 16)[:, 0]
            assert float(slots.max()) == exp, (n, offset, peak, float(slots.max()), exp)
            assert bool((bound >= 0).all())                            # no slot negative (and none NaN)


def run_net(net, x):
    with torch.no_grad():
        return [f.cpu() for f in net(x)]


@pytest.mark.parametrize("variant", ["filled", "zeroed"])
def test_shipped_network_at_8x8x8(device, variant):
    """B = 2 and each item as B = 1 against the fp64 CPU module: per returned feature max|got - ref| <= max(4 e32, 1e-6 max|ref|), e32
    the fp32 CPU forward's error against the same fp64 run, and elementwise_error <= 1e-4 beside it.

    Batch isolation: the module computes every bound itself (`absmax` of its input and of each decoder mean, and each layer's
    published max|y|) and offers no way to hand one in, so a B = 2 run and a B = 1 run of different items can differ in their
    scales; they are compared under the bar above, not bit for bit.  A batch of the SAME item twice has the bounds of that item
    alone: through the encoder's runners (the project's kernels only, no torch op whose algorithm could depend on B) both of its
    halves must equal the B = 1 result bit for bit, at every level down to the single voxel at 256 channels."""
    ref, f32 = C.net_reference(variant)
    x = C.net_input().to(device)
    net = C.build_shipped("device", variant).to(device)
    both = run_net(net, x)
    assert net.__dict__["_device_plan"] is not None and len(both) == 3
    singles = [run_net(net, x[b:b + 1].contiguous()) for b in range(2)]

    def encoder(v):
        outs, bound = [], None
        for level in net._device_runners()[0]:
            v, bound = net._run_level(level, v, bound)
            outs.append(v.cpu())
        return outs
    alone, twice = encoder(x[:1].contiguous()), encoder(torch.cat((x[:1], x[:1])))
    assert [tuple(t.shape[1:]) for t in alone] == [(32, 8, 8, 8), (64, 4, 4, 4), (128, 2, 2, 2), (256, 1, 1, 1)]
    for a, t in zip(alone, twice):
        assert torch.equal(t[:1], a) and torch.equal(t[1:], a) and bool(torch.isfinite(a).all())
    for i, (r, f) in enumerate(zip(ref, f32)):
        runs = [("B = 2", both[i], r, f)] + [(f"B = 1, item {b}", singles[b][i], r[b:b + 1], f[b:b + 1]) for b in range(2)]
        for label, got, rr, ff in runs:
            err, e32, bar = C.max_error(got, rr), C.max_error(ff, rr), C.net_bar(ff, rr)
            ew = elementwise_error(got, rr)
            print(f"{variant} feat{i} {label}: device {err:.3e}   fp32 CPU {e32:.3e}   max|ref| {float(rr.abs().max()):.3e}   "
                  f"bar {bar:.3e}   elementwise {ew:.3e}")
            assert got.shape == rr.shape and bool(torch.isfinite(got).all())
            assert err <= bar, (variant, i, label, err, bar)
            assert ew <= C.TOL, (variant, i, label, ew)
