"""Inputs, oracle, bar and host model of the 3D U-Net decoder-joint tests, shared by tests/test_unet_join_gpu.py (the device) and
tests/test_unet_join_cpu.py (the host model of the contract and its mutants, on these very tensors).

Every builder is cached and its tensors are never modified: a test that needs a variant clones."""
import functools

import torch
import torch.nn.functional as F

SUM_BAR = 8e-7                  # the family's bar against the largest sum|a||b| (tests/unet_cases.py)
ROUNDINGS = 6 * 2.0 ** -24      # one fp32 rounding per epilogue operation: the taps' sum, select's affine map (2), ReLU, sum, halving

# the fuse kernel's workgroup tile in FINE voxels (csrc/unet_join.hip: TX, TY, TZ); (3, 3, 17), fine 6 x 6 x 34, crosses all three at once
TILE = (4, 4, 32)
GEOMETRY_DIMS = [(1, 1, 1), (1, 3, 2), (2, 3, 5), (5, 4, 9), (3, 2, 17), (3, 3, 17)]
GEOMETRY_WIDTHS = (64, 32)
WIDTHS = [(32, 32), (64, 32), (32, 96), (128, 64), (256, 128), (96, 160), (256, 256)]
WIDTH_DIMS = (2, 3, 2)
STEPS = [1, 2, 4]
MODEL_CASES = [(64, 32, (5, 4, 9), 2), (128, 64, (2, 3, 5), 4), (256, 128, (2, 3, 2), 2)]      # (Cc, Cf, coarse dims, step)


def fine(dims):
    return tuple(2 * n for n in dims)


@functools.lru_cache(maxsize=None)
def make_case(cc, cf, dims, batch=1, step=1, seed=0):
    """randn activations, He-scaled weights, a folded-BatchNorm-like affine map and a 60 % observed mask at `step` times the fine
    resolution -> dict(xc, e, w_up, w_proj, scale, shift, observed); made once per shape and shared, never modified"""
    g = torch.Generator().manual_seed(1000 * seed + 7 * cc + 3 * cf + sum(dims) + 31 * batch + 101 * step)
    xc = torch.randn(batch, cc, *dims, generator=g)
    e = torch.randn(batch, cf, *fine(dims), generator=g)
    w_up = torch.randn(cf, cc, generator=g) * (2.0 / cc) ** 0.5
    w_proj = torch.randn(cf, cf, generator=g) * (2.0 / cf) ** 0.5
    scale = 1 + 0.1 * torch.randn(cf, generator=g)
    shift = 0.1 * torch.randn(cf, generator=g)
    observed = (torch.rand(batch, *(step * n for n in fine(dims)), generator=g) < 0.6).to(torch.uint8)
    return dict(xc=xc, e=e, w_up=w_up, w_proj=w_proj, scale=scale, shift=shift, observed=observed)


def sampled_mask(observed, step):
    """the reference's line: nearest F.interpolate of the float mask by 1 / step, != 0 -> bool [B, 1, X, Y, Z]"""
    m = observed.float()[:, None]
    return (F.interpolate(m, scale_factor=1 / step) if step > 1 else m) != 0


def _conv1(x, w):
    return F.conv3d(x, w.to(x.dtype).view(*w.shape[:2], 1, 1, 1))


def _chan(v, like):
    return v.to(like.dtype).view(1, -1, 1, 1, 1)


def oracle(xc, e, w_up, w_proj, scale, shift, observed=None, step=1, dtype=torch.float64):
    """the torch composition of the reference's lines in `dtype`: interpolate, 1x1x1 conv, conv of the skip, where, affine, ReLU, mean"""
    u = _conv1(F.interpolate(xc.to(dtype), scale_factor=2, mode="trilinear", align_corners=False), w_up)
    p = _conv1(e.to(dtype), w_proj)
    sel = p if observed is None else torch.where(sampled_mask(observed, step), p, u)
    if scale is not None:
        sel = sel * _chan(scale, sel) + _chan(shift, sel)
    return (u + sel.relu()) / 2


def magnitude(xc, e, w_up, w_proj, scale, shift, observed=None, step=1):
    """0.5 (A + |scale| where(mask, P, A)) with A = |w_up| . up(|xc|) and P = |w_proj| . |e| in fp64"""
    A = _conv1(F.interpolate(xc.double().abs(), scale_factor=2, mode="trilinear", align_corners=False), w_up.double().abs())
    P = _conv1(e.double().abs(), w_proj.double().abs())
    sel = P if observed is None else torch.where(sampled_mask(observed, step), P, A)
    return 0.5 * (A + (sel if scale is None else sel * _chan(scale.double().abs(), sel)))


def bar(mag, ref):
    return SUM_BAR * float(mag.max()) + ROUNDINGS * max(1.0, float(ref.abs().max()))


def max_error(got, ref):
    return float((got.double() - ref).abs().max())


def axis_taps(n, clamp=True, swap=False):
    """the contract's index formula along one axis of coarse length n -> (i0, i1, lam) over the 2n outputs.  clamp=False: the
    unclamped source position (taps outside the axis are marked -1: they read zero); swap: the two weights exchanged"""
    o = torch.arange(2 * n, dtype=torch.float64)
    src = o / 2 - 0.25
    if clamp:
        src = src.clamp(min=0)
    i0 = src.floor()
    lam = src - i0
    i0 = i0.long()
    i1 = i0 + 1
    if clamp:
        i1 = i1.clamp(max=n - 1)
    else:
        i0 = torch.where(i0 < 0, torch.full_like(i0, -1), i0)
        i1 = torch.where(i1 > n - 1, torch.full_like(i1, -1), i1)
    if swap:
        lam = torch.where(o > 0, 1 - lam, lam) if clamp else 1 - lam
    return i0, i1, lam


def upsample(v, clamp=True, swap=False):
    """x2 trilinear of v [B, C, X, Y, Z] by the explicit formula, one axis after the other (z first), in v's dtype"""
    for axis in (4, 3, 2):
        i0, i1, lam = axis_taps(v.shape[axis], clamp, swap)
        shape = [1] * 5
        shape[axis] = -1
        a, b = v.index_select(axis, i0.clamp(min=0)), v.index_select(axis, i1.clamp(min=0))
        a = a * (i0 >= 0).to(v.dtype).view(shape)
        b = b * (i1 >= 0).to(v.dtype).view(shape)
        lam = lam.to(v.dtype).view(shape)
        v = (1 - lam) * a + lam * b
    return v


MUTANTS = ["unclamped_border", "weights_swapped", "mask_ignored", "mask_without_step", "no_halving", "relu_before_affine"]


def host_model(xc, e, w_up, w_proj, scale, shift, observed=None, step=1, mutant=None, dtype=torch.float32):
    """the contract as the kernels compute it, in fp32: w_up on the COARSE grid, the explicit taps, the strided mask, the epilogue.
    mutant: one of MUTANTS, a plausible wrong reading of the contract"""
    v = _conv1(xc.to(dtype), w_up)
    u = upsample(v, clamp=mutant != "unclamped_border", swap=mutant == "weights_swapped")
    p = _conv1(e.to(dtype), w_proj)
    sel = p
    if observed is not None and mutant != "mask_ignored":
        X, Y, Z = e.shape[2:]
        m = observed[:, :X, :Y, :Z] if mutant == "mask_without_step" else observed[:, ::step, ::step, ::step]
        sel = torch.where(m[:, None] != 0, p, u)
    if mutant == "relu_before_affine":
        r = sel.relu() * _chan(scale, sel) + _chan(shift, sel)
    else:
        r = (sel * _chan(scale, sel) + _chan(shift, sel)).relu()
    return u + r if mutant == "no_halving" else (u + r) / 2


# ---- exactness: inputs on which fp32 has nothing to round
EXACT_CASES = [(64, 32, (3, 3, 17), 2), (32, 64, (3, 5, 4), 1), (32, 32, (1, 1, 1), 4)]


@functools.lru_cache(maxsize=None)
def exact_case(cc, cf, dims, step):
    """xc, e: integers of at most 10 bits times 2^-2 (|.| < 2^8); w_up, w_proj one-hot rows with +-2^k, k in {-1, 0, 1}; scale =
    +-2^k alike, shift an integer in [-3, 3].  Every product is exact; v = w_up . xc and p are below 2^9 in units of 2^-3; the
    eight taps weigh j / 64, so u and every partial sum of it are below 2^9 in units of 2^-9 (18 bits); scale * sel + shift is below
    2^11 in units of 2^-10 (21 bits); u + ReLU(.) is below 2^12 in units of 2^-10 (22 bits), and halving is exact.  Nothing is
    rounded in fp32 in any order of summation, so the result is the fp64 oracle's, bit for bit"""
    g = torch.Generator().manual_seed(5 + 13 * cc + 7 * cf + sum(dims))

    def ints(shape):
        return (torch.randint(0, 2 ** 10, shape, generator=g) * (2 * torch.randint(0, 2, shape, generator=g) - 1)).float() * 2.0 ** -2

    def one_hot(rows, cols):
        c = torch.arange(rows)
        w = torch.zeros(rows, cols)
        w[c, (5 * c + 3) % cols] = (1 - 2 * (c % 2)).float() * 2.0 ** ((c % 3) - 1).float()
        return w
    c = torch.arange(cf)
    scale = (1 - 2 * ((c // 2) % 2)).float() * 2.0 ** (((c // 3) % 3) - 1).float()
    shift = ((c % 7) - 3).float()
    observed = (torch.rand(1, *(step * n for n in fine(dims)), generator=g) < 0.6).to(torch.uint8)
    return dict(xc=ints((1, cc, *dims)), e=ints((1, cf, *fine(dims))), w_up=one_hot(cf, cc), w_proj=one_hot(cf, cf), scale=scale,
                shift=shift, observed=observed)
