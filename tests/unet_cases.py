"""Inputs, oracle and bars of the 3D U-Net convolution tests, shared by tests/test_unet_gpu.py, tests/test_unet_edges_gpu.py (the
device) and tests/test_unet_model_cpu.py (the host model of the arithmetic, tests/unet_model.py): the CPU test shows on these very
tensors that ideal f16x3 and an fp32 torch convolution pass every bar and that an f16x3 which loses a cross term does not.

Every builder is cached and its tensors are never modified: a test that needs a variant clones."""
import functools
import itertools

import torch
import torch.nn.functional as F

TOL = 1e-4                      # the project's parity bound (helpers.elementwise_error)
SUM_BAR = 8e-7                  # f16x3 against the largest sum|a||b| (tests/test_sparse_edges_gpu.py), up to a dot of 27 * 256
ROUNDINGS = 4 * 2.0 ** -24      # one fp32 rounding for each of the epilogue's three operations and the activation


@functools.lru_cache(maxsize=None)
def make_case(cin, cout, dims, batch=1, seed=0):
    """O(1) input and He-scaled weights, made once per shape and shared, never modified"""
    g = torch.Generator().manual_seed(1000 * seed + 7 * cin + 3 * cout + sum(dims) + 31 * batch)
    x = torch.randn(batch, cin, *dims, generator=g)
    w = torch.randn(cout, cin, 3, 3, 3, generator=g) * (2.0 / (27 * cin)) ** 0.5
    scale = 1 + 0.1 * torch.randn(cout, generator=g)
    shift = 0.1 * torch.randn(cout, generator=g)
    return x, w, scale, shift


def epilogue(y, scale=None, shift=None, residual=None, relu=False):
    """* scale[c] + shift[c], + residual, ReLU, in y's dtype"""
    if scale is not None:
        y = y * scale.to(y.dtype).view(1, -1, 1, 1, 1) + shift.to(y.dtype).view(1, -1, 1, 1, 1)
    if residual is not None:
        y = y + residual.to(y.dtype)
    return y.relu() if relu else y


def oracle(x, w, stride=1, scale=None, shift=None, residual=None, relu=False, dtype=torch.float64):
    return epilogue(F.conv3d(x.to(dtype), w.to(dtype), stride=stride, padding=1), scale, shift, residual, relu)


def magnitude(x, w, stride=1, scale=None, **_):
    """sum|a||b| of every output's dot product in fp64, carried through the epilogue: times |scale[c]|"""
    mag = F.conv3d(x.double().abs(), w.double().abs(), stride=stride, padding=1)
    return mag if scale is None else mag * scale.double().abs().view(1, -1, 1, 1, 1)


def sum_bar(mag, ref):
    """the bar of tests/test_sparse_edges_gpu.close(mag=...): 8e-7 of the largest sum|a||b| plus four fp32 roundings of the result"""
    return SUM_BAR * float(mag.max()) + ROUNDINGS * max(1.0, float(ref.abs().max()))


def max_error(got, ref):
    return float((got.double() - ref).abs().max()) if ref.numel() else 0.0


# ---- the comparisons of tests/test_unet_gpu.py that go through `check`, as (cin, cout, dims, stride, epilogue mode)
EDGE_DIMS = [(1, 1, 1), (1, 5, 3), (5, 7, 3), (9, 8, 17), (8, 8, 8), (12, 20, 8)]
WIDTHS = [(32, 64), (64, 32), (96, 96), (128, 256), (256, 256)]
WIDTH_DIMS = (4, 6, 5)
STRIDE2_WIDTHS = [(32, 64), (128, 256)]
STRIDE2_DIMS = [((5, 7, 3), (3, 4, 2)), ((6, 8, 4), (3, 4, 2)), ((1, 1, 1), (1, 1, 1)), ((12, 20, 8), (6, 10, 4))]
EPILOGUES = ["none", "affine", "affine_relu", "affine_residual_relu"]
EPILOGUE_SHAPE = (32, 64, (5, 7, 9))
# ---- stride 2 with Cout no multiple of 64: launch_conv3<2, 1, 1, 2>, the form no earlier test reached.  (7, 3, 3) is two boxes along x
NARROW_STRIDE2_WIDTHS = [(32, 32), (64, 32), (32, 96), (64, 96)]
NARROW_STRIDE2_DIMS = [(1, 1, 1), (5, 7, 3), (6, 8, 4), (4, 9, 17), (7, 3, 3)]


def epilogue_kw(mode, cin=EPILOGUE_SHAPE[0], cout=EPILOGUE_SHAPE[1], dims=EPILOGUE_SHAPE[2]):
    _, _, scale, shift = make_case(cin, cout, dims)
    res = torch.randn(1, cout, *dims, generator=torch.Generator().manual_seed(9))
    return dict(none={}, affine=dict(scale=scale, shift=shift), affine_relu=dict(scale=scale, shift=shift, relu=True),
                affine_residual_relu=dict(scale=scale, shift=shift, residual=res, relu=True))[mode]


def bar_cases():
    """(id, cin, cout, dims, kw of the oracle) of every comparison under the sum|a||b| bar"""
    out = [(f"edge-{d}", 32, 32, d, {}) for d in EDGE_DIMS]
    out += [(f"width-{ci}-{co}", ci, co, WIDTH_DIMS, {}) for ci, co in WIDTHS]
    out += [(f"stride2-{ci}-{co}-{d}", ci, co, d, dict(stride=2)) for ci, co in STRIDE2_WIDTHS for d, _ in STRIDE2_DIMS]
    out += [(f"epilogue-{m}", *EPILOGUE_SHAPE, epilogue_kw(m)) for m in EPILOGUES]
    out += [(f"narrow-stride2-{ci}-{co}-{d}", ci, co, d, dict(stride=2)) for ci, co in NARROW_STRIDE2_WIDTHS for d in NARROW_STRIDE2_DIMS]
    return out


# ---- exactness: inputs on which f16x3 has nothing to round
EXACT_WIDTHS = [(32, 32), (64, 64), (64, 96)]
EXACT_DIMS = [(9, 6, 11), (1, 1, 1)]
EXACT_KINDS = ["x_bits", "w_bits"]
EXACT_CASES = list(itertools.product(EXACT_KINDS, EXACT_WIDTHS, EXACT_DIMS, (1, 2)))


def _integers21(shape, g):
    """integers of up to 21 bits with random sign, the widest one present"""
    n = torch.randint(0, 2 ** 21, shape, generator=g) * (2 * torch.randint(0, 2, shape, generator=g) - 1)
    n.view(-1)[n.numel() // 2] = -(2 ** 21 - 1)
    return n.float()                                                   # 21 bits: exact in fp32


@functools.lru_cache(maxsize=None)
def exact_case(kind, cin, cout, dims):
    """output channel c has ONE nonzero weight, at tap c % 27 and input channel (5 c + 3) % cin, so every output is one product
    w * x at a shifted voxel (or a zero of the halo).  "x_bits": x = 21-bit integers * 2^-9, that weight = +-2^k, k in [-3, 3];
    "w_bits": the weight = a 21-bit integer * 2^-12, x = +-2^k.

    Why f16x3 is exact here: the power-of-two scale puts the largest |a| in [2^13, 2^14), so a 21-bit integer n becomes n u with
    the unit u >= 2^13 / 2^20 = 2^-7.  h = fp16(n u) keeps the leading 11 bits; the remainder is a multiple of u of magnitude at
    most half an ulp of h, 2^9 u, so it has at most 10 bits and its lowest bit u >= 2^-7 is far above the fp16 subnormal step
    2^-24: m holds it exactly and h + m = n u.  The other operand is a power of two: its h is exact and its m is 0.  The one
    product of an output is then (n u)(2^k s) = m * h' + h * h' with both terms exact in fp32 and their sum a 21-bit integer times a
    power of two, and every other term of the dot is an exact zero.  The result is w * x, bit for bit."""
    g = torch.Generator().manual_seed(77 + 13 * cin + 5 * cout + sum(dims) + (kind == "w_bits"))
    c = torch.arange(cout)
    tap, ci = c % 27, (5 * c + 3) % cin
    sign = (1 - 2 * (c % 2)).float()
    w = torch.zeros(cout, cin, 27)
    if kind == "x_bits":
        x = _integers21((1, cin, *dims), g) * 2.0 ** -9
        w[c, ci, tap] = sign * 2.0 ** ((c * 3) % 7 - 3).float()
    else:
        k = torch.randint(-3, 4, (1, cin, *dims), generator=g).float()
        x = (2 * torch.randint(0, 2, k.shape, generator=g) - 1).float() * 2.0 ** k
        w[c, ci, tap] = _integers21((cout,), g) * 2.0 ** -12
    return x, w.view(cout, cin, 3, 3, 3)


FAR_SHAPE = (32, 64, (5, 7, 9))                 # the case of test_power_of_two_scaling_is_exact
FAR_SCALES = [(60, 40), (-40, -30)]             # x * 2^px with w * 2^pw: the result is base * 2^(px + pw), bit for bit


# ---- wide dynamic range
WIDE_SHAPE = (64, 64, (9, 8, 17))
WIDE_GAIN = 2.0 ** 12


@functools.lru_cache(maxsize=None)
def wide_case():
    """randn with every channel of the corner voxel (0, 0, 0) multiplied by 2^12 -> (x, w, quiet), quiet: the output voxels whose
    3x3x3 neighbourhood misses that voxel (stride 1: any coordinate above 1)"""
    x, w, _, _ = make_case(*WIDE_SHAPE)
    x = x.clone()
    x[0, :, 0, 0, 0] *= WIDE_GAIN
    ix, iy, iz = torch.meshgrid(*(torch.arange(n) for n in WIDE_SHAPE[2]), indexing="ij")
    quiet = (ix > 1) | (iy > 1) | (iz > 1)
    return x, w, quiet.view(1, 1, *WIDE_SHAPE[2]).expand(1, WIDE_SHAPE[1], *WIDE_SHAPE[2])


def wide_margin(got, ref, mag, quiet):
    """the smallest of (element's bar) / (element's error) over the quiet outputs; the bar: 8e-7 of the element's own sum|a||b| plus
    four roundings of the element"""
    bar = SUM_BAR * mag + ROUNDINGS * ref.abs().clamp(min=1.0)
    err = (got.double() - ref).abs()
    return float((bar[quiet] / err[quiet].clamp(min=1e-300)).min())


# ---- absmax
ABSMAX_SIZES = [0, 1, 2, 3, 4, 5, 255, 1025, 2048 * 256 * 4 + 5]     # the last: eight trips of the grid-stride loop and a tail of 5
ABSMAX_OFFSETS = [0, 1, 2, 3]                                        # floats into the allocation: 0 is the vector path
ABSMAX_PEAKS = ["first", "last", "middle_negative", "tail_negative"]
GUARD = 4                                                             # floats kept in front of and behind the view


@functools.lru_cache(maxsize=8)
def _absmax_body(n):
    return torch.rand(n, generator=torch.Generator().manual_seed(n)) - 0.5


def absmax_case(n, offset, peak):
    """-> (allocation, start, expected max|view|): the view is allocation[start : start + n], start = GUARD + offset floats in (a
    fresh device allocation is aligned to far more than 16 bytes, GUARD floats are 16, so `offset` alone decides the alignment);
    |view| <= 0.5 but for one peak of magnitude 3; everything outside the view is 1e6 or -1e6, so a read outside it shows"""
    start = GUARD + offset
    alloc = torch.full((start + n + GUARD,), 1.0e6)
    alloc[1::2] = -1.0e6
    view = alloc[start:start + n]
    view.copy_(_absmax_body(n))
    if n:
        at, value = dict(first=(0, 3.0), last=(n - 1, 3.0), middle_negative=(n // 2, -3.0), tail_negative=(n - 1 - (n - 1) % 4, -3.0))[peak]
        view[at] = value
    return alloc, start, float(view.abs().max()) if n else 0.0


# ---- the shipped network
NET_VOLUME = (8, 8, 8)


def shipped_cfg():
    from projects.configs.mvsdetection._builders import backbone_3d_cfg
    cfg = backbone_3d_cfg()
    assert cfg["channels"] == [32, 64, 128, 256] and cfg["layers_down"] == [1, 2, 3, 4] and cfg["layers_up"] == [3, 2, 1]
    return cfg


def build_shipped(impl, variant):
    """backbone_3d_cfg() filled by unet_fixture.fill, eval mode.  variant "filled": as filled; "zeroed": bn2.weight exactly 0 on every
    second block in forward order, so its folded scale is 0 and the block is ReLU(shift + x)"""
    import projects.mvsdetection  # noqa: F401
    from projects.mvsdetection.models.backbone3d import BasicBlock3d
    from projects.mvsdetection.registry import build_backbone
    import unet_fixture as UF
    net = UF.fill(build_backbone(dict(shipped_cfg(), impl=impl))).eval().requires_grad_(False)
    if variant == "zeroed":
        blocks = [m for m in net.modules() if isinstance(m, BasicBlock3d)]
        assert len(blocks) == 16
        for m in blocks[1::2]:
            m.bn2.weight.zero_()
    return net


@functools.lru_cache(maxsize=None)
def net_input():
    """two O(1) items of 32 x 8 x 8 x 8: the levels are 8, 4, 2 and 1 voxels wide"""
    return torch.randn(2, 32, *NET_VOLUME, generator=torch.Generator().manual_seed(41))


@functools.lru_cache(maxsize=None)
def net_reference(variant):
    """-> (fp64 features, fp32 features) of the module on the CPU over the two-item input"""
    x = net_input()
    with torch.no_grad():
        ref = build_shipped("torch", variant).double()(x.double())
        f32 = build_shipped("torch", variant)(x)
    return ref, f32


def net_bar(f32, ref):
    """max(4 x the fp32 CPU forward's error against the fp64 run, 1e-6 max|ref|): the bar of tests/test_recon_gpu.bar_ok"""
    return max(4 * max_error(f32, ref), 1e-6 * float(ref.abs().max()))
