"""The host models of oracle/util_oracle.py checked on their own (no GPU): the hash is a bijection, the selection key orders
floats the way the model states, the models agree with independent restatements, and the NMS inputs of the GPU tests keep
their distance from every threshold."""
import numpy as np
import pytest
import torch

from oracle import post_oracle as PO
from oracle import util_oracle as U


def _hash_scalar(seed, i):
    """row_hash once more, in Python integers"""
    x = (i * 0x9E3779B1 + seed) & 0xFFFFFFFF
    x ^= x >> 16
    x = (x * 0x7FEB352D) & 0xFFFFFFFF
    x ^= x >> 15
    x = (x * 0x846CA68B) & 0xFFFFFFFF
    x ^= x >> 16
    return x


@pytest.mark.parametrize("seed", [0, 1, 0xFFFFFFFF, 0x9E3779B9])
def test_row_hash_is_a_bijection_on_a_million_rows(seed):
    h = U.row_hash(seed, np.arange(10**6))
    assert h.dtype == np.uint32 and len(np.unique(h)) == 10**6          # no ties: the kept set of a seed is unique
    for i in (0, 1, 2, 255, 65535, 999_999):
        assert int(h[i]) == _hash_scalar(seed, i)
    assert int(U.row_hash(seed, 0xFFFFFFFF)) == _hash_scalar(seed, 0xFFFFFFFF)


def test_select_seed_wraps():
    assert U.select_seed(5, 0) == 5
    assert U.select_seed(0, 1) == 0x9E3779B9
    assert U.select_seed(0xFFFFFFFF, 1) == 0x9E3779B8
    assert U.select_seed(3, 0xFFFFFFFF) == (3 - 0x9E3779B9) % 2**32
    assert U.select_seed(7, 7) == (7 + 7 * 0x9E3779B9) % 2**32


@pytest.mark.parametrize("cap,live,n_keep", [(1, 1, 1), (10, 10, 3), (10, 7, 7), (10, 7, 9), (10, 0, 4), (10, 15, 4), (5000, 3000, 2999)])
def test_sample_mask_model(cap, live, n_keep):
    m = U.sample_mask(cap, live, n_keep, seed=11)
    lv = min(live, cap)
    assert m.shape == (cap,) and m.dtype == np.uint8 and int(m.sum()) == min(lv, n_keep) and not m[lv:].any()
    h = np.array([_hash_scalar(11, i) for i in range(lv)], dtype=np.uint64)
    if 0 < n_keep < lv:
        assert h[m[:lv] == 1].max() < h[m[:lv] == 0].min()
    assert np.array_equal(U.sample_mask(cap, live, n_keep, 11, word=3), U.sample_mask(cap, live, n_keep, U.select_seed(11, 3)))
    if 0 < n_keep < lv and lv > 100:
        assert not np.array_equal(U.sample_mask(cap, live, n_keep, 11, word=3), m)


def test_select_key_is_ieee_total_order_descending_and_invertible():
    f = np.array([np.inf, 3e38, 1.0, 1e-45, 0.0, -0.0, -1e-45, -1.0, -3e38, -np.inf], dtype=np.float32)
    keys = U.select_key(U.score_bits(f))
    assert (np.diff(keys.astype(np.int64)) > 0).all()                    # strictly ascending keys for descending scores
    pos_nan, neg_nan = np.uint32(0x7FC00000), np.uint32(0xFFC00000)
    assert U.select_key(pos_nan) < keys[0] and U.select_key(neg_nan) > keys[-1]
    assert int(U.select_key(np.uint32(0x7FFFFFFF))) == 0 and int(U.select_key(np.uint32(0xFFFFFFFF))) == 0xFFFFFFFF
    rng = np.random.RandomState(0)
    k = rng.randint(0, 2**32, 100_000, dtype=np.uint64).astype(np.uint32)
    k[:4] = (0, 0xFFFFFFFF, 0x80000000, 0x7FFFFFFF)
    assert np.array_equal(U.select_key(U.score_bits(U.scores_from_keys(k))), k)
    # on finite distinct values the key order is the float order
    x = np.unique(rng.randn(5000).astype(np.float32))
    assert np.array_equal(np.argsort(U.select_key(U.score_bits(x)), kind="stable"), np.argsort(-x.astype(np.float64), kind="stable"))
    assert U.key_digits(0xFFFFFFFF) == (2047, 2047, 1023) and U.key_digits((5 << 21) | (7 << 10) | 9) == (5, 7, 9)


def test_topk_rows_model():
    rng = np.random.RandomState(1)
    x = rng.randn(3000).astype(np.float32)
    x[::5] = x[2]                                                            # ties -> smaller row first
    for live, k in ((3000, 1), (3000, 700), (2000, 700), (10, 700), (0, 3)):
        rows = U.topk_rows(x, live, k)
        n = min(live, k)
        assert len(rows) == n
        exp = torch.sort(torch.from_numpy(x[:live].copy()), descending=True, stable=True).indices[:n].numpy()
        assert np.array_equal(rows, exp)
    z = np.array([0.0, -0.0, 0.0, -0.0], dtype=np.float32)
    assert list(U.topk_rows(z, 4, 4)) == [0, 2, 1, 3]                        # -0.0 ranks below +0.0
    nan = np.array([1.0, np.nan, -np.inf, np.inf], dtype=np.float32)
    nan.view(np.uint32)[1] = 0x7FC00000
    assert list(U.topk_rows(nan, 4, 4)) == [1, 3, 0, 2]
    nan.view(np.uint32)[1] = 0xFFC00000
    assert list(U.topk_rows(nan, 4, 4)) == [3, 0, 2, 1]


def test_select_records_model():
    counts = np.array([0, 2, 0, 3, 1, 0], dtype=np.int64)
    off = np.concatenate(([0], np.cumsum(counts)))
    kept = np.arange(6 * 3 * 2, dtype=np.int32).reshape(6, 3, 2) + 100
    rec = U.select_records(off, kept, cap=6, live=6, n_keep=10, seed=0)      # everything kept, in row order
    assert rec[:, 0].tolist() == [1, 1, 3, 3, 3, 4] and not rec[:, 3].any()
    assert rec[:, 1].tolist() == [kept[1, 0, 1], kept[1, 1, 1], kept[3, 0, 1], kept[3, 1, 1], kept[3, 2, 1], kept[4, 0, 1]]
    assert rec[:, 2].tolist() == [kept[1, 0, 0], kept[1, 1, 0], kept[3, 0, 0], kept[3, 1, 0], kept[3, 2, 0], kept[4, 0, 0]]
    short = U.select_records(off, kept, cap=4, live=6, n_keep=10, seed=0)     # the capacity cuts ray 3 short and drops ray 4
    assert np.array_equal(short, rec[:4])
    some = U.select_records(off, kept, cap=6, live=6, n_keep=3, seed=5)
    m = U.sample_mask(6, 6, 3, 5)
    assert np.array_equal(some, rec[m == 1])


def test_suppression_bits_and_greedy_model():
    b = np.zeros((4, 7), dtype=np.float32)
    b[:, 3:6] = 1.0
    b[1, 0] = 0.5                        # IoU(0, 1) = 1/3
    b[2, 0] = 5.0                        # alone
    b[3, 0] = 0.75                       # IoU(0, 3) = 0.25 / 1.75, IoU(1, 3) = 0.75 / 1.25
    iou = U.pair_iou(b)
    np.testing.assert_allclose([iou[0, 1], iou[0, 3], iou[1, 3], iou[0, 2]], [1 / 3, 1 / 7, 0.6, 0.0], atol=1e-12)
    assert not np.tril(iou).any()
    assert U.suppression_bits(b, 0.3).ravel().tolist() == [0b0010, 0b1000, 0, 0]
    assert U.suppression_bits(b, 0.1).ravel().tolist() == [0b1010, 0b1000, 0, 0]
    assert U.greedy_keep(U.suppression_bits(b, 0.3)).tolist() == [0, 2, 3]
    assert U.greedy_keep(U.suppression_bits(b, 0.3)).tolist() == PO.nms(b, -np.arange(4.0), 0.3).tolist()
    assert abs(U.min_threshold_margin(b, 0.3) - (1 / 3 - 0.3)) < 1e-12
    many = U.nms_boxes(70, True, 3)
    bits = U.suppression_bits(many, 0.3)
    assert bits.shape == (70, 2) and np.array_equal(U.greedy_keep(bits), PO.nms(many, -np.arange(70.0), 0.3))


@pytest.mark.parametrize("rotated", [True, False], ids=["rotated", "axis"])
def test_nms_inputs_keep_their_margin_from_every_threshold(rotated):
    """every (n, kind, seed, thr) of tests/test_post_edges_gpu.py: no pairwise oracle IoU within 1e-4 of the threshold, five
    times the 2e-5 by which the float32 kernel may differ -- so the mask bits can be compared exactly"""
    for n in sorted(U.NMS_COUNTS, reverse=True):
        boxes, iou = U.nms_case(n, rotated)
        assert boxes.shape == (n, 7) and iou.shape == (n, n) and (rotated or not boxes[:, 6].any())
        for thr in U.NMS_THRESHOLDS:
            assert U.min_threshold_margin(boxes, thr, iou) >= U.NMS_MARGIN, (n, rotated, U.NMS_SEEDS[rotated], thr)
    full, iou = U.nms_case(max(U.NMS_COUNTS), rotated)
    assert np.array_equal(iou[:5, :5], U.pair_iou(full[:5]))
    for thr in U.NMS_THRESHOLDS:                                          # and the cases suppress something, but not all
        kept = len(U.greedy_keep(U.suppression_bits(full, thr, iou)))
        assert 3 < kept < len(full) - 3, (thr, kept)
