"""What the bars of tests/test_unet_gpu.py and tests/test_unet_edges_gpu.py can tell apart, established on the host: on the very
tensors the device tests use (tests/unet_cases.py), ideal f16x3 (tests/unet_model.py) and an fp32 torch convolution pass every
bar, and f16x3 with a lost cross term -- `wh * xm` missing, `wm * xh` missing, the weight planes swapped -- fails the exactness
cases and fails the sum|a||b| bar at every width.  A device kernel with such a slip therefore fails those tests; no GPU run is
needed to know it.

No input had to be changed for a mutant's sake: on the randn cases every mutant is more than 10 times outside the 8e-7 bar (15 times
at the longest dot, 27 * 256; 40 to 100 times at the shortest, 27 * 32)."""
import pytest
import torch

import unet_cases as C
import unet_model as M

BAR_CASES = C.bar_cases()


def test_scale_and_split_follow_f16x3_h():
    assert [M.scale_for(a) for a in (0.0, float("inf"), float("nan"), 3.5e38)] == [1.0] * 4
    assert M.scale_for(1.0) == 2.0 ** 13 and M.scale_for(0.99) == 2.0 ** 14 and M.scale_for(2.0 ** 13) == 1.0
    assert M.scale_for(2.0 ** -120) == 2.0 ** 100 and M.scale_for(2.0 ** 120) == 2.0 ** -100        # the clamp
    a = torch.randn(4096, generator=torch.Generator().manual_seed(1))
    s = M.scale_for(a.abs().max())
    assert 2.0 ** 13 <= float(a.abs().max()) * s < 2.0 ** 14
    h, m = M.split(a, s)
    rel = ((a.double() * s - h - m).abs() / (a.double() * s).abs())
    assert float(rel[a.abs() * s >= 2.0 ** -3].max()) <= 2.0 ** -22      # 2^-17 of the largest and up: 22 bits (f16x3.h)


@pytest.mark.parametrize("label,cin,cout,dims,kw", BAR_CASES, ids=[c[0] for c in BAR_CASES])
def test_sum_bar_passes_the_arithmetic_and_fails_every_mutant(label, cin, cout, dims, kw):
    x, w, _, _ = C.make_case(cin, cout, dims)
    ref, mag = C.oracle(x, w, **kw), C.magnitude(x, w, **kw)
    bar = C.sum_bar(mag, ref)
    ideal, fp32 = C.max_error(M.conv3(x, w, **kw), ref), C.max_error(C.oracle(x, w, dtype=torch.float32, **kw), ref)
    mutants = {name: C.max_error(M.conv3(x, w, mutant=name, **kw), ref) for name in M.MUTANTS}
    top = float(mag.max())
    print(f"{label}: of the largest sum|a||b|: ideal {ideal / top:.2e}   fp32 torch {fp32 / top:.2e}   "
          + "   ".join(f"{k} {v / top:.2e}" for k, v in mutants.items()) + f"   (bar {bar / top:.2e})")
    assert ideal <= bar and fp32 <= bar
    for name, err in mutants.items():
        assert err > bar, (label, name, err, bar)


def test_every_width_of_the_device_tests_is_among_the_bar_cases():
    widths = {(c[1], c[2]) for c in BAR_CASES}
    assert widths >= set(C.WIDTHS) | set(C.NARROW_STRIDE2_WIDTHS) | set(C.STRIDE2_WIDTHS) | {(32, 32), C.EPILOGUE_SHAPE[:2]}
    assert {c[1] * 27 for c in BAR_CASES} >= {27 * 32, 27 * 256}         # the shortest and the longest dot of the kernel


@pytest.mark.parametrize("kind,widths,dims,stride", C.EXACT_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_exactness_cases_are_exact_for_the_arithmetic_and_not_for_a_mutant(kind, widths, dims, stride):
    x, w = C.exact_case(kind, *widths, dims)
    ref = C.oracle(x, w, stride=stride)
    exp = ref.float()
    assert torch.equal(exp.double(), ref)                                # one product per output: the oracle itself is exact in fp32
    assert int((w != 0).sum()) == widths[1] and float(x.abs().max()) > 0
    assert torch.equal(M.conv3(x, w, stride=stride).float(), exp)
    assert torch.equal(C.oracle(x, w, stride=stride, dtype=torch.float32), exp)
    # the operand that carries the bits decides which cross term the case needs.  Swapped weight planes compute wh xh + wm xh + wm xm:
    # they lose wh * xm, which is nonzero only where x has a low half
    fails = dict(x_bits=("drop_hm", "swap_planes"), w_bits=("drop_mh",))[kind]
    for name in fails:
        assert not torch.equal(M.conv3(x, w, stride=stride, mutant=name).float(), exp), name
    # (1, 1, 1) under either stride: 27 * cin taps reach the one voxel, so only the channels whose tap is the centre are nonzero
    if dims == (1, 1, 1):
        assert [int(c) for c in exp.flatten().nonzero().flatten()] == [c for c in range(widths[1]) if c % 27 == 13]


def test_every_mutant_fails_an_exactness_case():
    caught = {name for kind, name in (("x_bits", "drop_hm"), ("w_bits", "drop_mh"), ("x_bits", "swap_planes"))
              for widths in C.EXACT_WIDTHS
              if not torch.equal(M.conv3(*C.exact_case(kind, *widths, C.EXACT_DIMS[0]), mutant=name).float(),
                                 C.oracle(*C.exact_case(kind, *widths, C.EXACT_DIMS[0])).float())}
    assert caught == set(M.MUTANTS)


@pytest.mark.parametrize("px,pw", C.FAR_SCALES)
def test_scales_far_apart_leave_the_result_a_power_of_two_away(px, pw):
    x, w, _, _ = C.make_case(*C.FAR_SHAPE)
    base = M.conv3(x, w)
    got = M.conv3(x * 2.0 ** px, w * 2.0 ** pw)
    assert torch.equal(got, base * 2.0 ** (px + pw))
    base32 = base.float()                                                # every output stays a normal fp32 number, so the cast commutes
    lo, hi = float(base32.abs()[base32 != 0].min()) * 2.0 ** (px + pw), float(base32.abs().max()) * 2.0 ** (px + pw)
    assert 2.0 ** -126 <= lo and hi < 2.0 ** 127
    assert torch.equal(got.float(), base32 * 2.0 ** (px + pw))
    f32 = C.oracle(x * 2.0 ** px, w * 2.0 ** pw, dtype=torch.float32)
    assert torch.equal(f32, C.oracle(x, w, dtype=torch.float32) * 2.0 ** (px + pw))


def test_wide_dynamic_range_leaves_the_per_element_bar_a_margin():
    """the scale is set by a voxel 2^12 above the rest; the quiet outputs are held to 8e-7 of their OWN sum|a||b|.  Measured here:
    the ideal arithmetic keeps a margin of 45 to that bar (f16x3.h suggested about 20) and fp32 torch one of 10; a mutant has none"""
    x, w, quiet = C.wide_case()
    ref, mag = C.oracle(x, w), C.magnitude(x, w)
    assert 0.9 < float(quiet.float().mean()) < 1.0 and float(mag[~quiet].min()) > 50 * float(mag[quiet].max())
    ideal = M.conv3(x, w)
    margin, margin32 = C.wide_margin(ideal, ref, mag, quiet), C.wide_margin(C.oracle(x, w, dtype=torch.float32), ref, mag, quiet)
    print(f"wide range: margin of the ideal arithmetic to the per-element bar {margin:.1f}, of fp32 torch {margin32:.1f}")
    assert margin >= 4 and margin32 >= 4
    assert C.max_error(ideal, ref) <= C.sum_bar(mag, ref)                # the loud corner under the usual bar
    for name in M.MUTANTS:
        assert C.wide_margin(M.conv3(x, w, mutant=name), ref, mag, quiet) < 1, name


@pytest.mark.parametrize("variant", ["filled", "zeroed"])
def test_shipped_network_bar_passes_the_arithmetic(variant):
    """the shipped architecture at 8 x 8 x 8 with its 3x3x3 convolutions computed by the model: inside max(4 e32, 1e-6 max|ref|) and
    inside 1e-4, per returned feature"""
    from helpers import elementwise_error
    ref, f32 = C.net_reference(variant)
    assert [tuple(f.shape) for f in ref] == [(2, 128, 2, 2, 2), (2, 64, 4, 4, 4), (2, 32, 8, 8, 8)]
    with torch.no_grad():
        got = M.model_network(C.build_shipped("torch", variant).double())(C.net_input().double())
    for i, (g, r, f) in enumerate(zip(got, ref, f32)):
        err, bar = C.max_error(g, r), C.net_bar(f, r)
        print(f"{variant} feat{i}: model {err:.3e}   fp32 {C.max_error(f, r):.3e}   max|ref| {float(r.abs().max()):.3e}   bar {bar:.3e}   "
              f"elementwise: model {elementwise_error(g, r):.3e}   fp32 {elementwise_error(f, r):.3e}")
        assert err <= bar and elementwise_error(g, r) <= C.TOL and elementwise_error(f, r) <= C.TOL
    if variant == "zeroed":
        net = C.build_shipped("torch", variant)
        assert sum(1 for k, v in net.state_dict().items() if k.endswith("bn2.weight") and not v.any()) == 8
