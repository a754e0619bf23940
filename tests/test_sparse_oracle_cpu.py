"""CPU suite: the sparse-half oracle (parity unpinned: ME is absent) is anchored on dense equivalences
(SURVEY.md 8c): sparse conv == conv3d on the densified grid at the active output sites, etc.; the decoder is
checked against the golden vectors produced by the reference's fcaf3d_head.py."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import sparse_oracle as SO

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def random_sparse(rng, D=10, occ=0.3, C=5, ts=1, batch=1, neg=False):
    cs = []
    for b in range(batch):
        m = rng.rand(D, D, D) < occ
        xyz = np.argwhere(m)
        rng.shuffle(xyz)
        if neg:
            xyz = xyz - D // 2
        cs.append(np.concatenate((np.full((len(xyz), 1), b), xyz * ts), axis=1))
    c = np.concatenate(cs).astype(np.int64)
    return c, rng.randn(len(c), C)


def densify(coords, feats, D, ts, fill=0.0, shift=0):
    g = np.full((feats.shape[1], D, D, D), fill)
    i = coords[:, 1:] // ts + shift
    g[:, i[:, 0], i[:, 1], i[:, 2]] = feats.T
    return torch.from_numpy(g)[None]


def dense_kernel(W, k):
    """W[kidx][ci][co] with kidx = ix + k*iy + k*k*iz  ->  [co, ci, kx, ky, kz]"""
    K, ci, co = W.shape
    return torch.from_numpy(W.reshape(k, k, k, ci, co).transpose(4, 3, 2, 1, 0).copy())   # (iz,iy,ix,..) -> (co,ci,ix,iy,iz)


@pytest.mark.parametrize("ts", [1, 2])
def test_conv_k3_stride1_equals_dense_conv3d(ts):
    rng = np.random.RandomState(0)
    c, f = random_sparse(rng, D=9, C=4, ts=ts)
    W = rng.randn(27, 4, 6)
    oc, of = SO.conv(c, f, W, 3, 1, ts)
    dense = F.conv3d(densify(c, f, 9, ts), dense_kernel(W, 3), padding=1)[0].numpy()
    i = oc[:, 1:] // ts
    np.testing.assert_allclose(of, dense[:, i[:, 0], i[:, 1], i[:, 2]].T, atol=1e-10)


def test_conv_k3_stride2_equals_dense_conv3d():
    rng = np.random.RandomState(1)
    c, f = random_sparse(rng, D=10, C=3, ts=1)
    W = rng.randn(27, 3, 5)
    oc, of = SO.conv(c, f, W, 3, 2, 1)
    assert (oc[:, 1:] % 2 == 0).all() and len(np.unique(SO._key(oc))) == len(oc)
    assert set(map(tuple, oc)) == set(map(tuple, np.concatenate((c[:, :1], c[:, 1:] // 2 * 2), axis=1)))
    dense = F.conv3d(densify(c, f, 10, 1), dense_kernel(W, 3), padding=1, stride=2)[0].numpy()
    i = oc[:, 1:] // 2
    np.testing.assert_allclose(of, dense[:, i[:, 0], i[:, 1], i[:, 2]].T, atol=1e-10)


def test_conv_k1_stride2_takes_only_the_coincident_input():
    rng = np.random.RandomState(2)
    c, f = random_sparse(rng, D=8, C=3)
    W = rng.randn(3, 4)
    oc, of = SO.conv(c, f, W, 1, 2, 1)
    look = SO.Lookup(c)
    idx = look(oc)
    exp = np.where((idx >= 0)[:, None], f[np.maximum(idx, 0)] @ W, 0.0)
    np.testing.assert_allclose(of, exp, atol=1e-12)


def test_maxpool_equals_dense_maxpool3d():
    rng = np.random.RandomState(3)
    c, f = random_sparse(rng, D=10, C=4, ts=2)
    oc, of = SO.max_pool(c, f, 2)
    dense = F.max_pool3d(densify(c, f, 10, 2, fill=-np.inf), 2, 2)[0].numpy()
    i = oc[:, 1:] // 4
    np.testing.assert_allclose(of, dense[:, i[:, 0], i[:, 1], i[:, 2]].T)


def test_generative_transpose_equals_dense_conv_transpose3d():
    rng = np.random.RandomState(4)
    c, f = random_sparse(rng, D=6, C=3, ts=4)
    W = rng.randn(8, 3, 5)
    oc, of = SO.conv_transpose_generative(c, f, W, 4)
    assert len(oc) == 8 * len(c) and len(np.unique(SO._key(oc))) == len(oc)
    wd = torch.from_numpy(W.reshape(2, 2, 2, 3, 5).transpose(3, 4, 2, 1, 0).copy())     # [ci, co, ix, iy, iz]
    dense = F.conv_transpose3d(densify(c, f, 6, 4), wd, stride=2)[0].numpy()
    i = oc[:, 1:] // 2
    np.testing.assert_allclose(of, dense[:, i[:, 0], i[:, 1], i[:, 2]].T, atol=1e-10)


def test_negative_coordinates_floor_toward_minus_infinity():
    c = np.array([[0, -1, -1, -1], [0, -2, 0, 3], [0, 1, 1, 1], [0, -3, -4, 5]])
    oc = SO.stride_coords(c, 2)
    assert list(map(tuple, oc)) == [(0, -2, -2, -2), (0, -2, 0, 2), (0, 0, 0, 0), (0, -4, -4, 4)]


def test_known_answers():
    # single active voxel: k3 conv sees only the centre tap (kidx 13)
    c = np.array([[0, 4, 4, 4]])
    f = np.array([[2.0]])
    W = np.arange(27, dtype=np.float64).reshape(27, 1, 1)
    _, o = SO.conv(c, f, W, 3, 1, 1)
    assert o[0, 0] == 2.0 * 13
    # kernel offset order: x fastest.  neighbour at +x is kidx 14, at +y kidx 16, at +z kidx 22
    for d, k in (((1, 0, 0), 14), ((0, 1, 0), 16), ((0, 0, 1), 22)):
        c2 = np.array([[0, 4, 4, 4], [0, 4 + d[0], 4 + d[1], 4 + d[2]]])
        f2 = np.array([[0.0], [1.0]])
        _, o = SO.conv(c2, f2, W, 3, 1, 1)
        assert o[0, 0] == k
    # 2x2x2 full block pooled to one site
    blk = np.array([[0, x, y, z] for x in (0, 1) for y in (0, 1) for z in (0, 1)])
    oc, o = SO.max_pool(blk, np.arange(8, dtype=np.float64).reshape(8, 1), 1)
    assert len(oc) == 1 and o[0, 0] == 7
    # two scenes never mix
    c3 = np.array([[0, 0, 0, 0], [1, 1, 0, 0]])
    _, o = SO.conv(c3, np.ones((2, 1)), np.ones((27, 1, 1)), 3, 1, 1)
    assert (o == 1).all()
    # union-add
    uc, uf = SO.union_add(np.array([[0, 0, 0, 0], [0, 2, 0, 0]]), np.array([[1.0], [2.0]]),
                          np.array([[0, 2, 0, 0], [0, 4, 0, 0]]), np.array([[10.0], [20.0]]))
    assert list(map(tuple, uc)) == [(0, 0, 0, 0), (0, 2, 0, 0), (0, 4, 0, 0)] and list(uf[:, 0]) == [1, 12, 20]
    # interpolation weights on the half-stride lattice are 1, 1/2, 1/4, 1/8; missing corners contribute 0
    sc = np.array([[0, 0, 0, 0], [0, 4, 0, 0]])
    out = SO.interpolate(sc, np.array([[1.0], [3.0]]), 4, np.array([[0, 0, 0, 0], [0, 2, 0, 0], [0, 2, 2, 0], [0, 2, 2, 2]]))
    np.testing.assert_allclose(out[:, 0], [1.0, 2.0, 1.0, 0.5])


def test_decode_matches_reference_golden():
    z = np.load(os.path.join(GOLDEN, "decode.npz"))
    pts = torch.from_numpy(z["points"])
    for nreg, yaw in ((6, "fcaf3d"), (8, "fcaf3d"), (8, "sin-cos"), (7, "naive")):
        box = SO.decode_boxes(pts, torch.from_numpy(z[f"pred_{nreg}_{yaw}"]), yaw)
        assert torch.equal(box, torch.from_numpy(z[f"box_{nreg}_{yaw}"]))


def test_compute_centerness_matches_reference_golden():
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from projects.mvsdetection.models.fcaf3d_head import compute_centerness
    z = np.load(os.path.join(GOLDEN, "decode.npz"))
    assert torch.equal(compute_centerness(torch.from_numpy(z["centerness_in"])), torch.from_numpy(z["centerness_out"]))


def test_fp32_torch_port_matches_the_fp64_oracle():
    """oracle/sparse_torch.py (the multi-threaded fp32 restatement timed as bench.py's cpu_baseline) against the fp64
    numpy oracle on a random surface-like point set: every level's coordinate set identical, head outputs close"""
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from oracle import sparse_torch as ST
    from projects.mvsdetection.models.fcaf3d_backbone import FCAF3DBackbone
    from projects.mvsdetection.models.fcaf3d_head import FCAF3DHead
    rng = np.random.RandomState(0)
    n = 4000
    uv = rng.randint(0, 160, size=(n, 2))
    z = (40 + 8 * np.sin(uv[:, 0] / 17.0) + rng.randint(0, 3, size=n)).astype(np.int64)
    coords = np.unique(np.concatenate((np.zeros((n, 1), dtype=np.int64), uv, z[:, None]), axis=1), axis=0)
    feats = rng.randn(len(coords), 8).astype(np.float32)
    torch.manual_seed(0)
    backbone = FCAF3DBackbone(8, 34).eval()
    head = FCAF3DHead(18, (64, 128, 256, 512), 128, 6, 0.01, 300, None, test_cfg=dict(nms_pre=50)).eval()
    backbone.init_weights()
    head.init_weights()
    lv64 = SO.backbone_forward(backbone, coords, feats)
    lv32 = ST.backbone_forward(backbone, coords, feats)
    for (c64, f64, _), (cs32, f32) in zip(lv64, lv32):
        assert np.array_equal(c64, cs32.C.numpy())
        np.testing.assert_allclose(f32.numpy(), f64, rtol=2e-3, atol=2e-3)
    r64 = SO.head_forward(head, lv64)
    r32 = ST.head_forward(head, lv32)
    for a, b in zip(r64, r32):
        assert a["coords"].shape == tuple(b["coords"].shape)
        ka = np.lexsort(a["coords"].T[::-1])
        kb = np.lexsort(b["coords"].numpy().T[::-1])
        same = (a["coords"][ka] == b["coords"].numpy()[kb]).all(axis=1)
        assert same.mean() > 0.99              # ties at the pruning threshold may differ
        np.testing.assert_allclose(b["cls_score"].numpy()[kb][same], a["cls_score"][ka][same], rtol=5e-3, atol=5e-3)
    b32, s32 = ST.get_bboxes(head, r32)
    assert torch.isfinite(b32).all() and torch.isfinite(s32).all()


# ---- prepared weight images: the oracle's element orders ----------------------------------------------------------------------
IMAGE_SHAPES = [(1, 32, 4), (3, 64, 130), (27, 32, 32), (2, 12, 20)]


# fragment orders exist for Cin % 32 == 0 only (the entry points reject the rest)
@pytest.mark.parametrize("order,shape", [(o, s) for o in ("stage", "frag16", "frag32") for s in IMAGE_SHAPES
                                         if o == "stage" or s[1] % 32 == 0])
def test_weight_image_order_is_a_bijection_onto_the_padded_weights(order, shape):
    K, Ci, Co = shape
    Cp = SO.cout_padded(Co)
    assert Cp == -(-Co // 128) * 128 and Cp % 128 == 0 and 0 <= Cp - Co < 128
    idx = SO.weight_image_index(order, K, Ci, Co)
    assert idx.shape == (K * Ci * Cp,)
    live = idx[idx >= 0]
    assert np.array_equal(np.sort(live), np.arange(K * Ci * Co))              # each (k, cin, co < Cout) exactly once
    assert (idx[idx < 0] == -1).all() and (idx < 0).sum() == K * Ci * (Cp - Co)   # everything else is padding
    # second statement of the same orders, element by element: the index forms of include/cnrma.h (stage order, fragment tile
    # shapes) and of the layout comments in csrc/sparse.hip (lane -> channel and column inside a fragment tile); the oracle
    # builds its orders from reshapes and transposes instead
    t = np.arange(K * Ci * Cp)
    if order == "stage" and Ci % 32 == 0:
        c32, q = t % 32, t // 32
        co, q = q % Cp, q // Cp
        cin, k = (q % (Ci // 32)) * 32 + c32, q // (Ci // 32)
    elif order == "stage":
        cin, q = t % Ci, t // Ci
        co, k = q % Cp, q // Cp
    else:
        q = t >> 10
        tile, q = q % (Cp // 32), q // (Cp // 32)
        sl, k = q % (Ci // 32), q // (Ci // 32)
        if order == "frag16":
            j, lane, ks = t & 7, (t >> 3) & 63, (t >> 9) & 1
            cin = sl * 32 + 16 * ks + 8 * (lane >> 5) + j
        else:
            e, lane, i = t & 3, (t >> 2) & 63, (t >> 8) & 3
            cin = sl * 32 + 8 * i + 4 * (lane >> 5) + e
        co = tile * 32 + (lane & 31)
    assert np.array_equal(idx, np.where(co < Co, (k * Ci + cin) * Co + co, -1))


@pytest.mark.parametrize("kind", sorted(SO.WEIGHT_IMAGE_KINDS))
def test_weight_image_encodings_are_exact_and_padding_is_zero(kind):
    K, Ci, Co = 3, 64, 130
    order, enc = SO.WEIGHT_IMAGE_KINDS[kind]
    rng = np.random.default_rng(5)
    W = rng.standard_normal((K, Ci, Co)).astype(np.float32)
    img = SO.weight_image(kind, W)
    idx = SO.weight_image_index(order, K, Ci, Co)
    n = len(idx)
    src = np.where(idx >= 0, W.reshape(-1)[np.maximum(idx, 0)], np.float32(0))
    if enc == "f32":
        assert np.array_equal(img.view(np.float32), src)
        return
    planes = {"bf16": 1, "bf16x3": 3, "f16x2": 2}[enc]
    body = img[:2 * planes * n].view(np.uint16)
    body = body.reshape(planes, n) if order == "stage" else body.reshape(-1, planes, 1024).transpose(1, 0, 2).reshape(planes, n)
    assert (body[:, idx < 0] == 0).all()
    if enc == "f16x2":
        assert len(img) == 4 * n + 4 and img[4 * n:].view(np.float32)[0] == np.abs(W).max()
        scale = SO.f16_scale(np.abs(W).max())
        assert np.abs(W).max() * scale < 2.0 ** 14 <= np.abs(W).max() * scale * 2
        hi, lo = (p.view(np.float16).astype(np.float64) for p in body)
        assert np.abs(hi + lo - src.astype(np.float64) * float(scale)).max() <= 2.0 ** 14 * 2.0 ** -22      # two 11-bit pieces
    else:
        pieces = [(p.astype(np.uint32) << 16).view(np.float32).astype(np.float64) for p in body]
        if enc == "bf16x3":
            assert np.array_equal(sum(pieces), src.astype(np.float64))                                    # exact split
        else:
            assert np.abs(pieces[0] - src).max() <= np.abs(src).max() * 2.0 ** -8
    # transposed source: the image of W[K - 1 - k]^T
    W = rng.standard_normal((3, 64, 32)).astype(np.float32)
    Wt = np.ascontiguousarray(W[::-1].transpose(0, 2, 1))
    assert np.array_equal(SO.weight_image(kind, W, transpose=True, flip=True), SO.weight_image(kind, Wt))
    assert not np.array_equal(SO.weight_image(kind, W, transpose=True, flip=False), SO.weight_image(kind, Wt))


# ---------------------------------------------------------------------------------------------------------------------
# the oracle's training-mode BatchNorm and max-pool gradients against central differences of their own fp64 forward
# (what tests/test_sparse_backward_edges_gpu.py measures the HIP kernels against)
# ---------------------------------------------------------------------------------------------------------------------
def _central(f, a, h=1e-5):
    """d f() / d a by central differences, a perturbed in place element by element"""
    g = np.zeros_like(a)
    for i in np.ndindex(*a.shape):
        keep = a[i]
        a[i] = keep + h
        up = f()
        a[i] = keep - h
        g[i] = (up - f()) / (2 * h)
        a[i] = keep
    return g


@pytest.mark.parametrize("act", [None, "relu", "elu"])
@pytest.mark.parametrize("with_res", [False, True])
@pytest.mark.parametrize("n,C", [(5, 4), (9, 8)])
def test_batch_norm_train_backward_matches_finite_differences(n, C, with_res, act):
    from helpers import clear_of_kink
    rng = np.random.RandomState(100 * n + C)
    eps = 1e-5
    w = 0.5 + rng.rand(C)
    x, b, r = clear_of_kink(rng.randn(n, C) * 2 + 1, w, rng.randn(C), eps, rng.randn(n, C) if with_res else None, act)
    x, b, r = x.astype(np.float64), b.astype(np.float64), None if r is None else r.astype(np.float64)
    G = rng.randn(n, C)
    y, st = SO.batch_norm_train(x, w, b, eps, r, act)
    assert act is None or np.abs(st["pre"]).min() > 0.04          # a step of 1e-5 crosses no kink
    np.testing.assert_allclose(st["mean"], x.mean(0), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(st["var"], x.var(0), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(y, {None: lambda v: v, "relu": SO.relu, "elu": SO.elu}[act](st["pre"]), rtol=0, atol=0)
    dx, dr, dw, db = SO.batch_norm_train_backward(x, w, b, eps, G, r, act)
    loss = lambda: float((SO.batch_norm_train(x, w, b, eps, r, act)[0] * G).sum())
    for got, arg in ((dx, x), (dw, w), (db, b)) + (((dr, r),) if with_res else ()):
        fd = _central(loss, arg)
        assert np.abs(got - fd).max() <= 1e-6 * np.abs(fd).max(), (np.abs(got - fd).max(), np.abs(fd).max())
    assert (dr is None) == (not with_res)


@pytest.mark.parametrize("n,C,ts", [(5, 4, 1), (9, 8, 2)])
def test_max_pool_backward_matches_finite_differences(n, C, ts):
    rng = np.random.RandomState(n)
    xyz = np.stack(np.meshgrid(*[np.arange(-1, 2)] * 3, indexing="ij"), axis=-1).reshape(-1, 3)
    c = np.concatenate((np.zeros((n, 1), dtype=np.int64), xyz[rng.permutation(27)[:n]] * ts), axis=1)
    f = rng.randn(n, C)
    oc, out = SO.max_pool(c, f, ts)
    assert 1 < len(oc) < n                                         # windows with several children and more than one window
    s = np.sort(f, axis=0)
    assert (s[1:] - s[:-1]).min() > 1e-4                           # distinct values: a step of 1e-5 changes no argmax
    G = rng.randn(*out.shape)
    got = SO.max_pool_backward(c, f, G, ts)
    fd = _central(lambda: float((SO.max_pool(c, f, ts)[1] * G).sum()), f)
    assert np.abs(got - fd).max() <= 1e-6 * np.abs(fd).max()
    assert (np.count_nonzero(got, axis=0) == len(oc)).all()        # one child per window and channel takes the gradient
