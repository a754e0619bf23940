"""The head tail of csrc/points.hip and the box kernels of csrc/nms.hip at their edge sizes: decode and scores at the block
boundary with every id form, saturating logits, the fused head tail with poisoned padding columns and its argument rules; the
NMS suppression mask bit for bit against the oracle's matrix at the 64-bit word boundaries, and the IoU kernels against closed
forms in float64 that do not share the clipping algorithm."""
import os

import numpy as np
import pytest
import torch

from helpers import GOLDEN
from oracle import post_oracle as PO
from oracle import util_oracle as U

pytestmark = pytest.mark.gpu

EINVAL = -22
CANARY = -7777
SIZES = [1, 255, 256, 257]                         # one row, and the 256-thread block boundary
MODES = {(6, "fcaf3d"): 0, (8, "fcaf3d"): 1, (8, "sin-cos"): 2, (7, "naive"): 3}


def _lib():
    from cnrma_amd import _lib
    return _lib


def _args(args):
    """tensors -> device pointers (the tensors stay referenced until the entry has returned)"""
    return [a.data_ptr() if isinstance(a, torch.Tensor) else a for a in args]


def _call(name, *args):
    assert _lib().call(name, *_args(args)) == 0


def _rc(name, *args):
    return getattr(_lib().load(), name)(*_args(args))


def _dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


# ---------------------------------------------------------------------------------------------------------------------
# decode
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden_decode():
    z = np.load(os.path.join(GOLDEN, "decode.npz"))
    return {k: z[k] for k in z.files}


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("nreg,yaw", list(MODES), ids=lambda v: str(v))
def test_decode_entries_against_the_reference_vectors(device, golden_decode, nreg, yaw, n):
    """cnrma_fcaf3d_decode_f32 and cnrma_fcaf3d_select_decode_f32 (ids None; ids descending with repeats) on the first n rows
    of the reference's vectors: both within the project's bounds of the reference, and bit-identical to one another"""
    from cnrma_amd import sparse as S
    z = golden_decode
    pts, pred, exp = _dev(z["points"][:n], device), _dev(z[f"pred_{nreg}_{yaw}"][:n], device), z[f"box_{nreg}_{yaw}"][:n]
    rng = np.random.RandomState(n)
    cls, ctr = _dev(rng.randn(n, 3).astype(np.float32), device), _dev(rng.randn(n, 1).astype(np.float32), device)
    box = S.decode_boxes(pts, pred, yaw)
    np.testing.assert_allclose(box.cpu().numpy(), exp, rtol=1e-5, atol=1e-5)
    sc_exp = (1 / (1 + np.exp(-cls.cpu().numpy().astype(np.float64)))) * (1 / (1 + np.exp(-ctr.cpu().numpy().astype(np.float64))))
    ids_np = np.concatenate((np.arange(n)[::-1], [n - 1, 0, n // 2, n // 2])).astype(np.int64)       # descending, then repeats
    for ids in (None, ids_np):
        rows = np.arange(n) if ids is None else ids
        b2, s2 = S.select_decode(None if ids is None else _dev(ids, device), cls, ctr, pred, pts, yaw)
        assert b2.shape == (len(rows), exp.shape[1]) and s2.shape == (len(rows), 3)
        np.testing.assert_allclose(b2.cpu().numpy(), exp[rows], rtol=1e-5, atol=1e-5)
        assert np.array_equal(_bits(b2), _bits(box)[rows]), "the two decode entries differ on the same rows"
        np.testing.assert_allclose(s2.cpu().numpy(), sc_exp[rows], rtol=0, atol=1e-6)


def test_decode_argument_rules(device):
    """every (mode, R) pair but the four the head produces is refused by both entries, and so are modes outside 0..3"""
    n = 4
    pts, reg = torch.zeros(n, 3, device=device), torch.ones(n, 9, device=device)
    cls, ctr = torch.zeros(n, 2, device=device), torch.zeros(n, 1, device=device)
    boxes, scores = torch.zeros(n, 7, device=device), torch.zeros(n, 2, device=device)
    st = _lib().stream()
    good = {(0, 6), (1, 8), (2, 8), (3, 7)}
    for mode in (-1, 0, 1, 2, 3, 4):
        for R in (5, 6, 7, 8, 9):
            want = 0 if (mode, R) in good else EINVAL
            assert _rc("cnrma_fcaf3d_decode_f32", pts.data_ptr(), reg.data_ptr(), R, n, mode, boxes.data_ptr(), st) == want, (mode, R)
            assert _rc("cnrma_fcaf3d_select_decode_f32", None, n, cls.data_ptr(), ctr.data_ptr(), reg.data_ptr(), pts.data_ptr(), 2, R,
                       mode, scores.data_ptr(), boxes.data_ptr(), st) == want, (mode, R)
    assert _rc("cnrma_fcaf3d_decode_f32", pts.data_ptr(), reg.data_ptr(), 6, -1, 0, boxes.data_ptr(), st) == EINVAL
    assert _rc("cnrma_fcaf3d_decode_f32", pts.data_ptr(), reg.data_ptr(), 6, 0, 0, boxes.data_ptr(), st) == 0


# ---------------------------------------------------------------------------------------------------------------------
# scores
# ---------------------------------------------------------------------------------------------------------------------
LOGITS = np.array([0.0, -0.0, 30.0, -30.0, 88.7, -88.7, 104.0, -104.0, np.inf, -np.inf], dtype=np.float32)


def _sigmoid64(x):
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-x.astype(np.float64)))


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("n_cls", [1, 18])
def test_scores_at_saturating_logits(device, n_cls, n):
    """sigmoid(cls) * sigmoid(centerness) against float64 within 1e-6, with every pair of +-0, +-30, +-88.7 (exp near
    FLT_MAX), +-104 (exp overflows) and +-inf among the logits: in [0, 1], never NaN; the max-only entry equals the row maximum
    of the full one bit for bit"""
    from cnrma_amd import sparse as S
    rng = np.random.RandomState(n + n_cls)
    i = np.arange(n)
    ctr = LOGITS[i % 10].reshape(n, 1).copy()
    cls = LOGITS[(i[:, None] // 10 + np.arange(n_cls)[None, :]) % 10].copy()
    plain = rng.rand(n, n_cls) < 0.3                                      # and ordinary logits between them
    cls[plain] = (rng.randn(n, n_cls) * 3).astype(np.float32)[plain]
    exp = _sigmoid64(cls) * _sigmoid64(ctr)
    s, mx = S.class_scores(_dev(cls, device), _dev(ctr, device))
    s, mx = s.cpu().numpy(), mx.cpu().numpy()
    assert not np.isnan(s).any() and (s >= 0).all() and (s <= 1).all()
    err = float(np.abs(s.astype(np.float64) - exp).max())
    print(f"scores n={n} n_cls={n_cls}: largest |error| against float64 {err:.3e}")
    assert err <= 1e-6
    assert np.array_equal(mx.view(np.uint32), s.max(axis=1).view(np.uint32))
    only = S.max_scores(_dev(cls, device), _dev(ctr, device))
    assert np.array_equal(_bits(only), s.max(axis=1).view(np.uint32))


# ---------------------------------------------------------------------------------------------------------------------
# the fused head tail
# ---------------------------------------------------------------------------------------------------------------------
def _head_post(device, y, coords, R, n_cls, scale, vs):
    """the C entry with canaries behind every output"""
    n, ldy = y.shape
    outs = [torch.full((n * w + 16,), float(CANARY), dtype=torch.float32, device=device) for w in (1, R, n_cls, 1, 3)]
    sc = torch.tensor([scale], dtype=torch.float32, device=device)
    _call("cnrma_fcaf3d_head_post_f32", _dev(y, device), ldy, _dev(coords, device), n, R, n_cls, sc.data_ptr(),
          float(vs), *[o.data_ptr() for o in outs], _lib().stream())
    res = []
    for o, w in zip(outs, (1, R, n_cls, 1, 3)):
        a = o.cpu().numpy()
        assert (a[n * w:] == CANARY).all(), "head_post wrote behind an output"
        res.append(a[:n * w].reshape(n, w))
    return res


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("pad", [0, 5], ids=["ldy_min", "ldy_padded_nan"])
@pytest.mark.parametrize("R", [6, 7, 8])
def test_head_post_copies_exactly_and_ignores_the_padding(device, R, pad, n):
    """y = [centerness | reg (R) | cls | padding]: centerness, the class columns, their maximum, the tail of bbox_pred and
    points = float32(coords) * float32(voxel size) bit for bit; exp(scale * reg[:6]) within 1e-6 relative of float64; NaN in the
    padding columns reaches no output; negative coordinates"""
    n_cls = 18
    rng = np.random.RandomState(10 * n + R)
    ldy = 1 + R + n_cls + pad
    y = rng.randn(n, ldy).astype(np.float32)
    y[:, 1 + R + n_cls:] = np.nan
    coords = rng.randint(-300, 0, (n, 4)).astype(np.int32)
    coords[0, 1:] = (-32768, 0, 32767)
    scale, vs = np.float32(1.37), np.float32(0.01)
    cen, box, cls, mx, pts = _head_post(device, y, coords, R, n_cls, scale, vs)
    for a in (cen, box, cls, mx, pts):
        assert not np.isnan(a).any()
    u = lambda a: np.ascontiguousarray(a).view(np.uint32)
    assert np.array_equal(u(cen), u(y[:, :1])) and np.array_equal(u(cls), u(y[:, 1 + R:1 + R + n_cls]))
    assert np.array_equal(u(mx[:, 0]), u(y[:, 1 + R:1 + R + n_cls].max(axis=1)))
    assert np.array_equal(u(box[:, 6:]), u(y[:, 7:1 + R]))
    assert np.array_equal(u(pts), u(coords[:, 1:].astype(np.float32) * vs))
    exp = np.exp((y[:, 1:7] * scale).astype(np.float64))                 # the float32 product, then exp in float64
    rel = float((np.abs(box[:, :6].astype(np.float64) - exp) / exp).max())
    print(f"head_post n={n} R={R}: largest relative error of the exp columns {rel:.3e}")
    assert rel <= 1e-6


def test_head_post_argument_rules(device):
    n, n_cls = 4, 3
    y = torch.zeros(n, 16, device=device)
    coords = torch.zeros(n, 4, dtype=torch.int32, device=device)
    sc = torch.ones(1, device=device)
    outs = [torch.zeros(n * 9, device=device) for _ in range(5)]

    def rc(ldy, R, nc, rows=n):
        return _rc("cnrma_fcaf3d_head_post_f32", y.data_ptr(), ldy, coords.data_ptr(), rows, R, nc, sc.data_ptr(), 0.01,
                   *[o.data_ptr() for o in outs], _lib().stream())
    for R in (6, 7, 8):
        assert rc(1 + R + n_cls, R, n_cls) == 0 and rc(16, R, n_cls) == 0
        assert rc(1 + R + n_cls - 1, R, n_cls) == EINVAL                   # ldy too small by one column
    for R in (5, 0, -1):
        assert rc(16, R, n_cls) == EINVAL
    assert rc(16, 6, 0) == EINVAL and rc(16, 6, 3, rows=-1) == EINVAL and rc(16, 6, 3, rows=0) == 0


# ---------------------------------------------------------------------------------------------------------------------
# NMS: the suppression mask
# ---------------------------------------------------------------------------------------------------------------------
def _nms_mask(device, boxes, thr, rotated):
    """cnrma_nms_mask_f32 into a buffer prefilled with ones, 8 canary words behind it"""
    n = len(boxes)
    words = (n + 63) // 64
    buf = torch.full((n * words + 8,), -1, dtype=torch.int64, device=device)
    _call("cnrma_nms_mask_f32", _dev(boxes, device), n, float(thr), int(rotated), buf.data_ptr(), _lib().stream())
    got = buf.cpu().numpy()
    assert (got[n * words:] == -1).all(), "the mask kernel wrote behind its matrix"
    return got[:n * words].view(np.uint64).reshape(n, words)


@pytest.mark.parametrize("thr", U.NMS_THRESHOLDS)
@pytest.mark.parametrize("n", U.NMS_COUNTS)
@pytest.mark.parametrize("rotated", [True, False], ids=["rotated", "axis"])
def test_nms_mask_bits_equal_the_oracle_matrix(device, rotated, n, thr):
    """box counts on both sides of the 64-bit word boundaries; no pair of these boxes is within 1e-4 of a threshold
    (tests/test_util_oracle_cpu.py), so a float32 IoU within 2e-5 of the oracle decides every bit the same way"""
    from cnrma_amd import postprocess as PP
    boxes, iou = U.nms_case(n, rotated)
    exp = U.suppression_bits(boxes, thr, iou)
    got = _nms_mask(device, boxes, thr, rotated)
    assert np.array_equal(got, exp), np.argwhere(got != exp)[:8]
    for i in range(n):                                                      # on and below the diagonal everything is zero
        w, b = i >> 6, i & 63
        assert not got[i, :w].any() and not (int(got[i, w]) & ((2 << b) - 1)), i
    scores = -np.arange(n, dtype=np.float32)                                # the boxes are in score order
    keep = PP.nms_single_class(_dev(boxes if rotated else boxes[:, :6], device), _dev(scores, device), thr, rotated).cpu().numpy()
    assert np.array_equal(keep, U.greedy_keep(exp))
    if n <= 65 or thr == 0.3:                                               # the oracle's own greedy pass: all but 128 and 129
        assert np.array_equal(keep, PO.nms(boxes, scores, thr))            # boxes at 0.1 and 0.5, which cost it a second each


@pytest.mark.parametrize("rotated", [True, False], ids=["rotated", "axis"])
def test_nms_threshold_is_strict(device, rotated):
    """a unit square inside a 2 x 1 box: IoU = 0.5 exactly, in float32 as in float64 (every coordinate and product is a small
    dyadic number).  IoU > thr suppresses, IoU == thr does not -- not even the IoU of 1 of identical boxes at thr = 1"""
    b = np.zeros((3, 7), dtype=np.float32)
    b[0, 3:6] = (2, 1, 1)
    b[1, 0], b[1, 3:6] = 0.5, (1, 1, 1)
    b[2] = b[1]
    assert PO.iou(b[0], b[1], mode3d=False) == 0.5
    assert _nms_mask(device, b, 0.5, rotated)[:, 0].tolist() == [0, 0b100, 0]
    below = float(np.nextafter(np.float32(0.5), np.float32(0)))
    assert _nms_mask(device, b, below, rotated)[:, 0].tolist() == [0b110, 0b100, 0]
    assert _nms_mask(device, b, 1.0, rotated)[:, 0].tolist() == [0, 0, 0]


# ---------------------------------------------------------------------------------------------------------------------
# IoU against closed forms
# ---------------------------------------------------------------------------------------------------------------------
ATOL = 2e-5


def _iou(device, a, b, rotated, mode3d):
    from cnrma_amd import postprocess as PP
    out = PP.box_iou(_dev(a.astype(np.float32), device), _dev(b.astype(np.float32), device), rotated=rotated, mode3d=mode3d)
    got = out.cpu().numpy()
    assert got.shape == (len(a), len(b)) and not np.isnan(got).any()
    return got.astype(np.float64)


def _aabb_iou(a, b, mode3d):
    """closed form for boxes without yaw, float64: products of interval overlaps"""
    a, b = a.astype(np.float64)[:, None, :], b.astype(np.float64)[None, :, :]
    def overlap(c, s):
        return np.maximum(np.minimum(a[..., c] + a[..., s] / 2, b[..., c] + b[..., s] / 2)
                          - np.maximum(a[..., c] - a[..., s] / 2, b[..., c] - b[..., s] / 2), 0)
    inter = overlap(0, 3) * overlap(1, 4)
    va, vb = a[..., 3] * a[..., 4], b[..., 3] * b[..., 4]
    if mode3d:
        inter, va, vb = inter * overlap(2, 5), va * a[..., 5], vb * b[..., 5]
    return inter / np.maximum(va + vb - inter, 1e-8)


def _flat_boxes(rng, n):
    b = np.zeros((n, 7), dtype=np.float32)
    b[:, :3] = rng.rand(n, 3) * 2.5
    b[:, 3:6] = 0.3 + rng.rand(n, 3) * 1.2
    return b


def _moved(b, theta, shift):
    """the boxes turned by theta about the z axis through the origin, then shifted"""
    c, s = np.cos(theta), np.sin(theta)
    out = b.astype(np.float64).copy()
    out[:, 0] = c * b[:, 0] - s * b[:, 1] + shift[0]
    out[:, 1] = s * b[:, 0] + c * b[:, 1] + shift[1]
    out[:, 2] += shift[2]
    out[:, 6] += theta
    return out


def _close(got, exp, what):
    err = float(np.abs(got - exp).max())
    print(f"IoU {what}: largest |error| against the closed form {err:.3e}")
    assert err <= ATOL, what


@pytest.mark.parametrize("mode3d", [False, True], ids=["bev", "3d"])
@pytest.mark.parametrize("na,nb", [(1, 257), (255, 1), (256, 3), (257, 2), (40, 37)])
def test_iou_of_unrotated_boxes_in_every_guise(device, na, nb, mode3d):
    """boxes without yaw have a closed form.  The axis-aligned kernel, the rotated kernel at yaw 0, the rotated kernel at yaw
    pi/2 with dx and dy swapped, and the rotated kernel after a joint turn and shift of both boxes must all give it; and
    IoU(a, b) = IoU(b, a)"""
    rng = np.random.RandomState(na * 1000 + nb)
    a, b = _flat_boxes(rng, na), _flat_boxes(rng, nb)
    exp = _aabb_iou(a, b, mode3d)
    assert (exp > 0.05).any() or na * nb < 10
    _close(_iou(device, a, b, False, mode3d), exp, "axis-aligned kernel")
    _close(_iou(device, a, b, True, mode3d), exp, "rotated kernel, yaw 0")
    _close(_iou(device, b, a, True, mode3d).T, exp, "rotated kernel, arguments swapped")
    qa, qb = a.copy(), b.copy()
    for q in (qa, qb):
        q[:, [3, 4]] = q[:, [4, 3]]
        q[:, 6] = np.pi / 2
    _close(_iou(device, qa, qb, True, mode3d), exp, "rotated kernel, yaw pi/2 with dx and dy swapped")
    for theta, shift in ((0.3, (0.5, -1.0, 0.25)), (-2.0, (-3.0, 2.0, -1.0)), (np.pi / 4, (0.0, 0.0, 0.0))):
        _close(_iou(device, _moved(a, theta, shift), _moved(b, theta, shift), True, mode3d), exp, "rotated kernel, joint turn and shift")


@pytest.mark.parametrize("mode3d", [False, True], ids=["bev", "3d"])
def test_iou_of_a_box_inside_another_is_the_size_ratio(device, mode3d):
    """a small box inside a large one, both at any yaw: IoU = area ratio (volume ratio in 3D mode)"""
    rng = np.random.RandomState(12)
    n = 257
    big = np.zeros((n, 7))
    big[:, :3] = rng.rand(n, 3) * 4 - 2
    big[:, 3:6] = 2.0 + rng.rand(n, 3)
    big[:, 6] = rng.uniform(-3.2, 3.2, n)
    small = np.zeros((n, 7))
    small[:, :3] = big[:, :3] + rng.uniform(-0.3, 0.3, (n, 3))        # circumradius <= 0.36, offset <= 0.43: inside half-width 1
    small[:, 3:6] = 0.1 + rng.rand(n, 3) * 0.4
    small[:, 6] = rng.uniform(-3.2, 3.2, n)
    big, small = big.astype(np.float32), small.astype(np.float32)
    k = 6 if mode3d else 5
    ratio = np.prod(small[:, 3:k].astype(np.float64), axis=1) / np.prod(big[:, 3:k].astype(np.float64), axis=1)
    _close(np.diag(_iou(device, small, big, True, mode3d)), ratio, "small box inside a large one")
    _close(np.diag(_iou(device, big, small, True, mode3d)), ratio, "large box around a small one")


@pytest.mark.parametrize("mode3d", [False, True], ids=["bev", "3d"])
@pytest.mark.parametrize("rotated", [True, False], ids=["rotated", "axis"])
def test_iou_of_touching_and_empty_boxes_is_zero(device, rotated, mode3d):
    """boxes that share only an edge or only a corner, and boxes of zero size: 0, never NaN"""
    unit = np.array([[0.5, 0.5, 0.5, 1, 1, 1, 0]])
    touch = np.array([[1.5, 0.5, 0.5, 1, 1, 1, 0], [0.5, 1.5, 0.5, 1, 1, 1, 0], [-0.5, 0.5, 0.5, 1, 1, 1, 0],     # an edge
                      [1.5, 1.5, 0.5, 1, 1, 1, 0], [-0.5, -0.5, 0.5, 1, 1, 1, 0], [1.5, -0.5, 0.5, 1, 1, 1, 0]])  # a corner
    _close(_iou(device, unit, touch, rotated, mode3d), np.zeros((1, 6)), "touching boxes")
    _close(_iou(device, touch, unit, rotated, mode3d), np.zeros((6, 1)), "touching boxes")
    empty = np.array([[0.5, 0.5, 0.5, 0, 0, 0, 0], [0.5, 0.5, 0.5, 0, 1, 1, 0], [0.5, 0.5, 0.5, 1, 0, 1, 0], [0.5, 0.5, 0.5, 0, 0, 1, 0.7],
                      [7.0, 7.0, 7.0, 0, 0, 0, 0]])
    both = np.concatenate((unit, empty))
    _close(_iou(device, empty, both, rotated, mode3d), np.zeros((5, 6)), "zero-size boxes")
    _close(_iou(device, both, empty, rotated, mode3d), np.zeros((6, 5)), "zero-size boxes")
    flat = np.array([[0.5, 0.5, 0.5, 1, 1, 0, 0]])                         # no height: empty in 3D, the unit square in BEV
    _close(_iou(device, flat, unit, rotated, mode3d), np.full((1, 1), 0.0 if mode3d else 1.0), "a box without height")
