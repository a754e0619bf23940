"""csrc/util.hip and cnrma_select_rows_f32 at their edge sizes, each against its exact host model (oracle/util_oracle.py or
numpy itself): the hashed sampler and its device seed word, the radix top-k select with the threshold on every kind of
digit boundary, the per-ray record selection, the scans on both sides of every switch between kernels, the fp64 sum, the
layout pass on both of its paths, the range check, the byte fill and the row copy.  Bit for bit unless a test says otherwise.
The tests own their output buffers (prefilled, with canary words behind them), so they go through the C entries."""
import math

import numpy as np
import pytest
import torch

from oracle import rma_oracle as O
from oracle import util_oracle as U

pytestmark = pytest.mark.gpu

EINVAL = -22
CANARY = -7777
POISON = 3e38             # a dead score: it would win every select that read it


def _lib():
    from cnrma_amd import _lib
    return _lib


def _args(args):
    """tensors -> device pointers.  Pass a buffer made on the spot as the tensor, never as its .data_ptr(): the tensor must
    stay referenced until the entry has returned, or the allocator hands its memory to the next buffer of the same call"""
    return [a.data_ptr() if isinstance(a, torch.Tensor) else a for a in args]


def _call(name, *args):
    """the C entry; raises unless it returns 0"""
    assert _lib().call(name, *_args(args)) == 0


def _rc(name, *args):
    """the C entry's return code, whatever it is"""
    return getattr(_lib().load(), name)(*_args(args))


def _dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _word(v, device):
    """one 32-bit device word holding v (signed or unsigned)"""
    v = int(v) & 0xFFFFFFFF
    return torch.tensor([v - (1 << 32) if v >= (1 << 31) else v], dtype=torch.int32, device=device)


def _sample_ws(device):
    return torch.empty(_lib().load().cnrma_sample_workspace_bytes(), dtype=torch.uint8, device=device)


def _scan_ws(n, device):
    return torch.empty(_lib().load().cnrma_scan_workspace_bytes(n), dtype=torch.uint8, device=device)


def _stream():
    return _lib().stream()


# ---------------------------------------------------------------------------------------------------------------------
# the sampler
# ---------------------------------------------------------------------------------------------------------------------
def _sample(device, cap, live, n_keep, seed, word=None):
    """cnrma_sample_mask into a mask prefilled with 0xFF with 64 canary bytes behind it"""
    buf = torch.full((cap + 64,), 0xFF, dtype=torch.uint8, device=device)
    m_dev = _word(live, device)
    sd = _word(word, device) if word is not None else None
    _call("cnrma_sample_mask", m_dev.data_ptr(), cap, n_keep, seed, sd.data_ptr() if sd is not None else None,
          buf.data_ptr(), _sample_ws(device), _stream())
    out = buf.cpu().numpy()
    assert (out[cap:] == 0xFF).all(), "the sampler wrote behind its mask"
    return out[:cap]


# (capacity, live, n_keep): one row; one block's stride (2048 rows) and its neighbours; more than one block; a live word of 0,
# below and above the capacity (it must act as the capacity); n_keep around the live count; more blocks than the grid cap
SAMPLER_CASES = [(1, 1, 1), (2, 2, 1), (255, 255, 100), (2047, 2047, 2046), (2048, 2048, 1), (2049, 2049, 2048), (70001, 70001, 1),
                 (70001, 50000, 20000), (70001, 0, 5), (70001, 80000, 300), (5000, 3000, 2999), (5000, 3000, 3000),
                 (5000, 3000, 3001), (2_200_000, 2_200_000, 500_000)]


@pytest.mark.parametrize("seed", [0, 1, 0xFFFFFFFF], ids=lambda s: f"seed{s:x}")
@pytest.mark.parametrize("cap,live,n_keep", SAMPLER_CASES, ids=lambda v: str(v))
def test_sample_mask_keeps_the_rows_of_the_model(device, cap, live, n_keep, seed):
    exp = U.sample_mask(cap, live, n_keep, seed)
    got = _sample(device, cap, live, n_keep, seed)
    assert np.array_equal(got, exp), (int(got.sum()), int(exp.sum()), np.nonzero(got != exp)[0][:8])
    assert np.array_equal(_sample(device, cap, live, n_keep, seed), got)            # and again: the same rows


@pytest.mark.parametrize("word", [0, 1, 7, 0xFFFFFFFF], ids=lambda w: f"word{w:x}")
@pytest.mark.parametrize("cap,live,n_keep", [(2049, 2049, 2048), (5000, 3000, 2999), (70001, 50000, 20000)], ids=lambda v: str(v))
def test_sample_mask_seed_word_folds_into_the_seed(device, cap, live, n_keep, word):
    """seed_dev, the word that gives every graph replay a fresh subset: the rows of the model at the folded seed, the rows of a
    call without the word at that seed, and other rows than word 0 gives"""
    for seed in (0, 1, 0xFFFFFFFF):
        got = _sample(device, cap, live, n_keep, seed, word)
        assert np.array_equal(got, U.sample_mask(cap, live, n_keep, seed, word)), (seed, word)
        assert np.array_equal(got, _sample(device, cap, live, n_keep, U.select_seed(seed, word))), (seed, word)
        assert np.array_equal(got, _sample(device, cap, live, n_keep, seed, word)), (seed, word)
        if word != 0:
            assert not np.array_equal(got, _sample(device, cap, live, n_keep, seed, 0)), (seed, word)


# ---------------------------------------------------------------------------------------------------------------------
# the top-k select
# ---------------------------------------------------------------------------------------------------------------------
def _topk_mask(device, scores, live, k):
    n = len(scores)
    buf = torch.full((n + 64,), 0xFF, dtype=torch.uint8, device=device)
    s = _dev(np.asarray(scores, dtype=np.float32), device)
    _call("cnrma_topk_mask_f32", s.data_ptr(), _word(live, device), n, k, buf.data_ptr(),
          _sample_ws(device), _stream())
    out = buf.cpu().numpy()
    assert (out[n:] == 0xFF).all(), "the select wrote behind its mask"
    return out[:n]


def _topk_indices(device, scores, live, k):
    n = len(scores)
    buf = torch.full((k + 8,), CANARY, dtype=torch.int64, device=device)
    s = _dev(np.asarray(scores, dtype=np.float32), device)
    _call("cnrma_topk_indices_f32", s.data_ptr(), _word(live, device), n, k, buf.data_ptr(),
          _sample_ws(device), _stream())
    out = buf.cpu().numpy()
    assert (out[k:] == CANARY).all(), "the select wrote behind out[k]"
    return out[:k]


def _check_topk(device, scores, live, k, indices=True):
    """both entries against the model: the mask holds exactly the model's rows, the index list holds them in the model's order
    with zeros behind min(live, k)"""
    n = len(scores)
    rows = U.topk_rows(scores, live, k)
    exp_mask = np.zeros(n, dtype=np.uint8)
    exp_mask[rows] = 1
    got = _topk_mask(device, scores, live, k)
    assert np.array_equal(got, exp_mask), ("mask", n, live, k, np.nonzero(got != exp_mask)[0][:8])
    if indices and k <= 1024:
        exp = np.zeros(k, dtype=np.int64)
        exp[:len(rows)] = rows
        got = _topk_indices(device, scores, live, k)
        assert np.array_equal(got, exp), ("indices", n, live, k, np.nonzero(got != exp)[0][:8])
    return rows


def _poisoned(scores, live):
    s = np.array(scores, dtype=np.float32)
    s[live:] = POISON
    return s


@pytest.mark.parametrize("n", [1, 2, 1024, 1025, 2049, 70001])
def test_topk_shapes_against_the_model(device, n):
    """every k around the 64-lane, the 1024-slot and the tie-list sizes, with a live word of 0, 1, k - 1, k, k + 1; the scores
    are arbitrary bit patterns drawn from a pool a third of the rows large (ties everywhere), dead rows hold 3e38"""
    rng = np.random.RandomState(n)
    pool = rng.randint(0, 2**32, max(1, n // 3), dtype=np.uint64).astype(np.uint32)
    scores = U.scores_from_keys(pool[rng.randint(0, len(pool), n)])
    for k in (1, 2, 63, 64, 65, 1023, 1024, 1025):
        for live in sorted({min(max(v, 0), n) for v in (0, 1, k - 1, k, k + 1)}):
            _check_topk(device, _poisoned(scores, live), live, k)


_DIGIT_MAX = (2047, 2047, 1023)
_DIGIT_SHIFT = (21, 10, 0)
_MID = (1000, 1000, 500)


def _keys_around_digit(p, d, rng):
    """keys whose digit of pass p is d - 1, d or d + 1 (23, 37 and 29 rows; the digits of the earlier passes are fixed, those of
    the later ones random), with 17 rows in front of them all and 40 behind when p > 0.  Returns (keys, rows in front of bin
    d, rows in bin d, largest key of bin d)"""
    def make(d0_delta, dp, cnt):
        """dp None: digit 0 is _MID[0] + d0_delta, the rest random; else the digits before pass p are _MID, that of pass p is dp"""
        dig = [np.full(cnt, _MID[q]) for q in range(3)]
        dig[0] = dig[0] + d0_delta
        if dp is not None:
            dig[p] = np.full(cnt, dp)
        for q in range(1 if dp is None else p + 1, 3):
            dig[q] = rng.randint(0, _DIGIT_MAX[q] + 1, cnt)
        return ((dig[0].astype(np.uint64) << 21) | (dig[1].astype(np.uint64) << 10) | dig[2].astype(np.uint64)).astype(np.uint32)
    groups, front = [], 0
    if p > 0:
        groups += [make(-1, None, 17), make(+1, None, 40)]
        front += 17
    if d > 0:
        groups.append(make(0, d - 1, 23))
        front += 23
    groups.append(make(0, d, 37))
    if d < _DIGIT_MAX[p]:
        groups.append(make(0, d + 1, 29))
    keys = np.concatenate(groups)
    rng.shuffle(keys)
    prefix = sum(_MID[q] << _DIGIT_SHIFT[q] for q in range(p))
    bin_hi = prefix | (d << _DIGIT_SHIFT[p]) | ((1 << _DIGIT_SHIFT[p]) - 1)
    return keys, front, 37, bin_hi


@pytest.mark.parametrize("d", ["0", "7", "8", "max"])
@pytest.mark.parametrize("p", [0, 1, 2], ids=lambda p: f"pass{p}")
def test_topk_threshold_on_a_digit_boundary(device, p, d):
    """the threshold key's digit of pass p is 0, the last bin of a thread's eight (7), the first of the next thread's (8) or the
    last bin (2047; 1023 in the last pass); k puts the cumulative count of that bin one above `need`, exactly at `need` (the
    threshold is the bin's last row), and makes the threshold the bin's first row"""
    d = _DIGIT_MAX[p] if d == "max" else int(d)
    keys, front, in_bin, bin_hi = _keys_around_digit(p, d, np.random.RandomState(100 * p + d))
    scores = U.scores_from_keys(keys)
    n = len(keys)
    for k, above in ((front + in_bin - 1, 1), (front + in_bin, 0), (front + 1, in_bin - 1)):
        thr = int(np.sort(keys)[k - 1])
        assert U.key_digits(thr)[p] == d and all(U.key_digits(thr)[q] == _MID[q] for q in range(p))
        assert int(np.count_nonzero(keys <= bin_hi)) - k == above           # cumulative count through the bin against need
        _check_topk(device, scores, n, k)
        _check_topk(device, np.concatenate((scores, np.full(50, POISON, np.float32))), n, k)


def test_topk_extreme_keys(device):
    """key 0 (digit 0 in all three passes) and key 0xFFFFFFFF (the last digit of all three) as the threshold"""
    rng = np.random.RandomState(7)
    keys = rng.randint(1, 2**32 - 1, 3000, dtype=np.uint64).astype(np.uint32)
    keys[[5, 1700]] = 0
    keys[[9, 2100]] = 0xFFFFFFFF
    scores = U.scores_from_keys(keys)
    assert _check_topk(device, scores, 3000, 1).tolist() == [5]
    assert _check_topk(device, scores, 3000, 2).tolist() == [5, 1700]
    assert 2100 not in _check_topk(device, scores, 3000, 2999, indices=False)
    assert 9 in _check_topk(device, scores, 3000, 2999, indices=False)


@pytest.mark.parametrize("kind", ["all_negative", "mixed_sign"])
def test_topk_signs(device, kind):
    rng = np.random.RandomState(3)
    x = rng.randn(5000).astype(np.float32)
    if kind == "all_negative":
        x = -np.abs(x) - np.float32(1e-3)
    x[::9] = x[4]
    for k in (1, 64, 1000, 1024, 4999):
        _check_topk(device, _poisoned(x, 4500), 4500, k)


def test_topk_all_scores_equal(device):
    rows = _check_topk(device, np.full(70001, 0.25, np.float32), 70001, 1000)
    assert rows.tolist() == list(range(1000))


def test_topk_more_than_256_ties_across_the_cut(device):
    """600 rows share the threshold score, the cut falls inside them and inside the live rows; the dead rows hold 3e38"""
    rng = np.random.RandomState(4)
    n, live = 2049, 1500
    x = rng.rand(n).astype(np.float32) * 0.4
    x[rng.permutation(live)[:100]] = 0.9
    tie = np.sort(rng.permutation(np.nonzero(x[:live] < 0.5)[0])[:600])
    x[tie] = 0.5
    x = _poisoned(x, live)
    for k in (101, 400, 699, 700):
        rows = _check_topk(device, x, live, k)
        assert sorted(set(rows) & set(tie)) == list(tie[:k - 100])


def test_topk_signed_zeros_and_nans_rank_by_bit_pattern(device):
    """-0.0 ranks below +0.0 although it sits at the smaller row; a NaN with a clear sign bit ranks above +inf, one with a set
    sign bit below -inf"""
    z = np.array([5.0, -0.0, 0.0, -1.0, -2.0], dtype=np.float32)
    assert _check_topk(device, z, 5, 2).tolist() == [0, 2]
    assert _check_topk(device, z, 5, 3).tolist() == [0, 2, 1]
    x = np.array([1.0, np.inf, 0.0, -np.inf, 2.0, 3.0], dtype=np.float32)
    x.view(np.uint32)[2] = 0x7FC00000
    x.view(np.uint32)[4] = 0xFFC00000
    assert _check_topk(device, x, 6, 1).tolist() == [2]
    assert _check_topk(device, x, 6, 2).tolist() == [2, 1]
    assert _check_topk(device, x, 6, 5).tolist() == [2, 1, 5, 0, 3]
    assert _check_topk(device, x, 6, 6).tolist() == [2, 1, 5, 0, 3, 4]


def test_topk_indices_takes_at_most_1024(device):
    """k = 1025: the C entry refuses, the Python wrapper goes through the mask and still returns the model's rows"""
    from cnrma_amd import sparse as S
    rng = np.random.RandomState(5)
    n = 2049
    x = rng.permutation(n).astype(np.float32) - 1000.0                       # distinct, both signs
    s = _dev(x, device)
    out = torch.full((1025 + 8,), CANARY, dtype=torch.int64, device=device)
    assert _rc("cnrma_topk_indices_f32", s.data_ptr(), _word(n, device), n, 1025, out.data_ptr(),
               _sample_ws(device), _stream()) == EINVAL
    assert bool((out == CANARY).all())
    for live in (n, 1300, 1025, 1024, 700):
        xs = _dev(_poisoned(x, live), device)
        rows = U.topk_rows(x, live, 1025)
        exp = np.zeros(1025, dtype=np.int64)
        exp[:len(rows)] = rows
        assert np.array_equal(S.topk_indices(xs, 1025, _word(live, device)).cpu().numpy(), exp), live
        exp_mask = np.zeros(n, dtype=np.uint8)
        exp_mask[rows] = 1
        assert np.array_equal(S.topk_mask(xs, 1025, _word(live, device)).cpu().numpy(), exp_mask), live


# ---------------------------------------------------------------------------------------------------------------------
# the sampler over per-ray records
# ---------------------------------------------------------------------------------------------------------------------
def _record_table(kind, rng):
    R = 300
    if kind == "one_ray":                                    # one ray owns every row
        counts = np.zeros(R, dtype=np.int32)
        counts[137] = 50
        slots = 50
    else:                                                    # 0 .. 9 rows each, empty rays at the start and at the end
        counts = rng.randint(0, 10, R).astype(np.int32)
        counts[:3] = 0
        counts[-4:] = 0
        counts[150] = 9
        slots = 9
    kept = rng.randint(-2**31, 2**31 - 1, (R, slots, 2)).astype(np.int32)
    return counts, kept


@pytest.mark.parametrize("over", [0, 7], ids=["live_eq_cap", "live_above_cap"])
@pytest.mark.parametrize("kind", ["mixed", "one_ray"])
def test_select_records_against_the_model(device, kind, over):
    counts, kept = _record_table(kind, np.random.RandomState(6))
    R, slots = kept.shape[:2]
    off = np.concatenate(([0], np.cumsum(counts))).astype(np.int32)
    total = int(off[-1])
    m_cap = total - over                                     # the live word (the total) equals the capacity, or exceeds it
    M = min(total, m_cap)
    d_off, d_kept, m_dev = _dev(off, device), _dev(kept, device), _word(total, device)
    for n_keep in (1, M // 3, M, M + 5):
        for seed, word in ((0, None), (0xFFFFFFFF, 7)):
            rec_cap = min(m_cap, n_keep)
            rec = torch.full((rec_cap + 4, 4), CANARY, dtype=torch.int32, device=device)
            n_sel = torch.full((1 + 4,), CANARY, dtype=torch.int32, device=device)
            cnt = torch.empty(R, dtype=torch.int32, device=device)
            roff = torch.empty(R + 1, dtype=torch.int32, device=device)
            sd = _word(word, device) if word is not None else None
            _call("cnrma_rma_select_records", d_off.data_ptr(), R, d_kept.data_ptr(), slots, m_dev.data_ptr(), m_cap, n_keep, seed,
                  sd.data_ptr() if sd is not None else None, _sample_ws(device), cnt.data_ptr(), roff.data_ptr(),
                  _scan_ws(R, device), rec_cap,
                  rec.data_ptr(), n_sel.data_ptr(), _stream())
            exp = U.select_records(off, kept, m_cap, total, n_keep, seed, word)
            got, ns = rec.cpu().numpy(), n_sel.cpu().numpy()
            assert len(exp) == min(M, n_keep) and ns[0] == len(exp) and (ns[1:] == CANARY).all(), (n_keep, seed, ns[0], len(exp))
            assert np.array_equal(got[:len(exp)], exp), (n_keep, seed)
            assert (got[rec_cap:] == CANARY).all(), "records written behind rec_cap"


# ---------------------------------------------------------------------------------------------------------------------
# the scans
# ---------------------------------------------------------------------------------------------------------------------
# nothing; one item; whole tiles and one item more behind the single-launch size (32 768); 2048 tiles, the last size at which
# every block adds up the tile sums itself, and one item more: the form with the tile-offset pass
SCAN_SIZES = [0, 1, 34816, 34817, 4_194_304, 4_194_305]


def _scan_patterns(n, value, rng, random_hi):
    z = np.zeros(n, dtype=np.int64)
    small = n <= 100_000                                     # the 4 M sizes run the patterns that reach their last tiles
    if small:
        yield "zeros", z
    yield "ones", z + 1
    yield "random", rng.randint(0, random_hi, n).astype(np.int64)
    for name, at in (("first", 0), ("last", n - 1), ("tile_end", 2047), ("tile_start", 2048), ("last_tile_start", (n - 1) // 2048 * 2048)):
        if 0 <= at < n and (small or not name.startswith("tile_")):
            one = z.copy()
            one[at] = value
            yield name, one


def _exclusive_scan(device, x):
    n = len(x)
    d_in = _dev(np.asarray(x, dtype=np.int32), device) if n else torch.zeros(1, dtype=torch.int32, device=device)
    out = torch.full((n + 1 + 16,), CANARY, dtype=torch.int32, device=device)
    _call("cnrma_exclusive_scan_i32", d_in.data_ptr(), out.data_ptr(), n, _scan_ws(n, device), _stream())
    got = out.cpu().numpy()
    assert (got[n + 1:] == CANARY).all(), "the scan wrote behind out[n]"
    return got[:n + 1]


def _mask_to_index(device, m):
    n = len(m)
    d_in = _dev(np.asarray(m, dtype=np.uint8), device) if n else torch.zeros(1, dtype=torch.uint8, device=device)
    sel = torch.full((n + 16,), CANARY, dtype=torch.int32, device=device)
    n_sel = torch.full((1 + 4,), CANARY, dtype=torch.int32, device=device)
    _call("cnrma_mask_to_index", d_in.data_ptr(), sel.data_ptr(), n_sel.data_ptr(), n, _scan_ws(n, device), _stream())
    got, ns = sel.cpu().numpy(), n_sel.cpu().numpy()
    assert (got[n:] == CANARY).all() and (ns[1:] == CANARY).all(), "mask_to_index wrote behind its outputs"
    return got[:n], int(ns[0])


@pytest.mark.parametrize("n", SCAN_SIZES)
def test_exclusive_scan_against_cumsum(device, n):
    for name, x in _scan_patterns(n, 5, np.random.RandomState(n % 1000), 7):
        exp = np.concatenate(([0], np.cumsum(x, dtype=np.int64)))
        got = _exclusive_scan(device, x)
        assert np.array_equal(got.astype(np.int64), exp), (name, np.nonzero(got != exp)[0][:8])


def test_exclusive_scan_total_just_under_two_to_31(device):
    x = np.full(32769, 65000, dtype=np.int64)
    exp = np.concatenate(([0], np.cumsum(x, dtype=np.int64)))
    assert 2**31 - 2**25 < exp[-1] < 2**31
    assert np.array_equal(_exclusive_scan(device, x).astype(np.int64), exp)


@pytest.mark.parametrize("n", SCAN_SIZES)
def test_mask_to_index_against_cumsum(device, n):
    for name, m in _scan_patterns(n, 1, np.random.RandomState(n % 1000 + 1), 2):
        rank = np.cumsum(m, dtype=np.int64) - m
        got, total = _mask_to_index(device, m)
        assert total == int(m.sum()), (name, total)
        assert np.array_equal(got.astype(np.int64), np.where(m != 0, rank, -1)), name


# ---------------------------------------------------------------------------------------------------------------------
# the fp64 sum
# ---------------------------------------------------------------------------------------------------------------------
def _sum_f64(device, x):
    n = len(x)
    d_in = _dev(np.asarray(x, dtype=np.float64), device) if n else torch.zeros(1, dtype=torch.float64, device=device)
    out = torch.full((1 + 8,), float(CANARY), dtype=torch.float64, device=device)
    _call("cnrma_sum_f64", d_in.data_ptr(), out.data_ptr(), n, _scan_ws(n, device), _stream())
    got = out.cpu().numpy()
    assert (got[1:] == CANARY).all()
    return float(got[0])


# one wave, one block, the 2048 rows a block is given, the grid cap (1024 blocks of 2048 rows) and their neighbours
@pytest.mark.parametrize("n", [0, 1, 63, 64, 255, 256, 257, 2047, 2048, 2049, 2_097_152, 2_100_001])
def test_sum_f64_is_exact_on_integers(device, n):
    """integer-valued doubles below 2^20: every partial sum is below 2^53 and exact, so any summation order gives the integer"""
    x = np.random.RandomState(n % 999).randint(0, 2**20, n).astype(np.int64)
    if n:
        x[0] = x[-1] = 2**20 - 1
    assert _sum_f64(device, x.astype(np.float64)) == float(int(x.sum()))


def test_sum_f64_random_doubles_within_the_order_free_bound(device):
    """|sum - exact| <= (n - 1) * 2^-53 * sum|x|: the first-order bound of ANY order of n - 1 rounded additions"""
    n = 2_100_001
    x = np.random.RandomState(8).randn(n) * np.exp(np.random.RandomState(9).uniform(-20, 20, n))
    exact = math.fsum(x.tolist())
    bound = (n - 1) * 2.0**-53 * math.fsum(np.abs(x).tolist())
    err = abs(_sum_f64(device, x) - exact)
    print(f"sum_f64 random doubles: |error| {err:.3e}, bound {bound:.3e}")
    assert err <= bound


# ---------------------------------------------------------------------------------------------------------------------
# NCHW -> NHWC
# ---------------------------------------------------------------------------------------------------------------------
_HW = {1: (1, 1), 4: (2, 2), 60: (6, 10), 63: (7, 9), 64: (8, 8), 65: (5, 13), 68: (4, 17), 4100: (50, 82)}


def _layout(device, V, C, hw, offset=0):
    """arbitrary 32-bit patterns through the C entry (source `offset` floats into a larger buffer), compared as int32 with
    permute(0, 2, 3, 1): the pass only moves data; 16 canary words behind the output"""
    H, W = _HW[hw]
    n = V * C * H * W
    rng = np.random.RandomState(V * 1000 + C * 7 + hw)
    big = _dev(rng.randint(0, 2**32, n + offset + 4, dtype=np.uint64).astype(np.uint32).view(np.int32), device)
    src = big[offset:offset + n]
    out = torch.full((n + 16,), CANARY, dtype=torch.int32, device=device)
    assert src.data_ptr() % 16 == (4 * offset) % 16 and out.data_ptr() % 16 == 0
    _call("cnrma_nchw_to_nhwc_f32", src.data_ptr(), out.data_ptr(), V, C, H, W, _stream())
    exp = src.view(V, C, H, W).permute(0, 2, 3, 1).reshape(-1)
    assert bool((out[n:] == CANARY).all()), ("wrote behind the output", V, C, hw)
    assert torch.equal(out[:n], exp), (V, C, hw, offset)


@pytest.mark.parametrize("C", [4, 60, 64, 68, 132])
def test_nchw_to_nhwc_16_byte_path_only_moves_data(device, C):
    """C % 4 == 0, HW % 4 == 0, aligned pointers: channel tails (C < 64, C = 64 + 4, 2 x 64 + 4) with pixel tails"""
    for hw in (4, 60, 64, 68, 4100):
        for V in (1, 3):
            _layout(device, V, C, hw)


@pytest.mark.parametrize("C", [1, 31, 32, 33])
def test_nchw_to_nhwc_scalar_path_only_moves_data(device, C):
    """C or HW no multiple of 4 (C = 32 with HW = 64 is the one pair here that qualifies for the 16-byte path)"""
    for hw in (1, 63, 64, 65):
        for V in (1, 3):
            _layout(device, V, C, hw)


@pytest.mark.parametrize("C,hw", [(8, 64), (68, 68)])
def test_nchw_to_nhwc_misaligned_source_takes_the_scalar_path(device, C, hw):
    """C % 4 == 0 and HW % 4 == 0, but the source starts one float into its buffer: 16-byte loads would be misaligned"""
    _layout(device, 2, C, hw, offset=1)


# ---------------------------------------------------------------------------------------------------------------------
# the range check of a static replay
# ---------------------------------------------------------------------------------------------------------------------
INT_MIN, INT_MAX = -2**31, 2**31 - 1


def _range_case(n, rng):
    lo = rng.randint(-1000, 0, n).astype(np.int64)
    hi = rng.randint(0, 1000, n).astype(np.int64)
    v = rng.randint(-1300, 1300, n).astype(np.int64)
    v[0] = lo[0] - 1                                             # a violation at the first item ...
    v[-1] = hi[-1] + 1                                           # ... and at the last (the same item when n = 1)
    if n >= 16:
        v[1], v[2] = lo[1], hi[2]                                # on the bounds: no violations
        v[3], lo[3] = INT_MIN, INT_MIN
        v[4], hi[4] = INT_MAX, INT_MAX
        v[5], v[6] = INT_MIN, INT_MAX                            # violations
        lo[7], hi[7], v[7] = INT_MIN, INT_MAX, 0
        v[n - 2] = hi[n - 2]
    return v.astype(np.int32), lo.astype(np.int32), hi.astype(np.int32)


def _violations(device, v, lo, hi):
    out = torch.full((1 + 8,), CANARY, dtype=torch.int32, device=device)
    _call("cnrma_range_violations_i32", _dev(v, device), _dev(lo, device), _dev(hi, device),
          len(v), out.data_ptr(), _stream())
    got = out.cpu().numpy()
    assert (got[1:] == CANARY).all()
    return int(got[0])


@pytest.mark.parametrize("n", [1, 255, 256, 257, 4095, 4096])
def test_range_violations_against_numpy(device, n):
    v, lo, hi = _range_case(n, np.random.RandomState(n))
    exp = int(((v < lo) | (v > hi)).sum())
    assert exp >= 1 and _violations(device, v, lo, hi) == exp
    assert _violations(device, lo, lo, hi) == 0 and _violations(device, hi, lo, hi) == 0
    ok = np.clip(v, lo, hi)
    assert _violations(device, ok, lo, hi) == 0
    ok[-1] = hi[-1] + 1
    assert _violations(device, ok, lo, hi) == 1


def test_range_violations_argument_rules(device):
    buf = torch.zeros(4097, dtype=torch.int32, device=device)
    out = torch.full((1,), CANARY, dtype=torch.int32, device=device)
    for n in (0, 4097, -1):
        assert _rc("cnrma_range_violations_i32", buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), n, out.data_ptr(), _stream()) == EINVAL
    assert _rc("cnrma_range_violations_i32", None, buf.data_ptr(), buf.data_ptr(), 4, out.data_ptr(), _stream()) == EINVAL
    assert int(out[0]) == CANARY


def test_plan_status_kernel_and_torch_fallback_agree(device):
    """Plan.status() counts with the kernel up to 4096 watched words and with torch ops above: the same watches give the same
    count on both sides of the switch"""
    from cnrma_amd.plan import Plan
    v, lo, hi = _range_case(4096, np.random.RandomState(11))
    exp = int(((v < lo) | (v > hi)).sum())
    words = _dev(np.concatenate((v, [5])).astype(np.int32), device)
    for n_watch in (4096, 4097):                                   # the 4097th watch holds: 0 <= 5 <= 9
        p = Plan()
        for i in range(n_watch):
            p.watch(words[i:i + 1], int(lo[i]) if i < 4096 else 0, int(hi[i]) if i < 4096 else 9)
        assert int(p.status(device)[0]) == exp, n_watch
    assert int(Plan().status(device)[0]) == 0


# ---------------------------------------------------------------------------------------------------------------------
# the byte fill
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", [0, 4, 8, 12], ids=lambda s: f"ptr16+{s}")
def test_fill_bytes_fills_its_range_only(device, shift):
    """destination 16-byte aligned (shift 0) or 4- but not 16-byte aligned; canary bytes on both sides"""
    for n in (4, 12, 16, 252, 256, 260, (1 << 20) + 4):
        for byte in (0x00, 0xFF, 0xA5):
            buf = torch.full((64 + n + 64,), 0x3C, dtype=torch.uint8, device=device)
            assert buf.data_ptr() % 16 == 0
            at = 48 + shift
            _call("cnrma_fill_bytes_u8", buf.data_ptr() + at, byte, n, _stream())
            got = buf.cpu().numpy()
            assert (got[:at] == 0x3C).all() and (got[at + n:] == 0x3C).all(), (n, byte, "wrote outside its range")
            assert (got[at:at + n] == byte).all(), (n, byte)


def test_fill_bytes_argument_rules(device):
    buf = torch.full((64,), 0x3C, dtype=torch.uint8, device=device)
    assert _rc("cnrma_fill_bytes_u8", buf.data_ptr(), 0, 6, _stream()) == EINVAL              # odd size
    assert _rc("cnrma_fill_bytes_u8", buf.data_ptr() + 2, 0, 8, _stream()) == EINVAL          # odd pointer
    assert _rc("cnrma_fill_bytes_u8", None, 0, 8, _stream()) == EINVAL                        # no pointer
    assert _rc("cnrma_fill_bytes_u8", buf.data_ptr(), 0, 0, _stream()) == 0                   # nothing to do
    assert bool((buf == 0x3C).all())


# ---------------------------------------------------------------------------------------------------------------------
# the row copy of switch_pointcloud
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [1, 3, 13, 64])
@pytest.mark.parametrize("M", [1, 255, 70001])
def test_select_rows_is_bit_exact(device, M, C):
    """one float32 add per coordinate, a copy per feature; M = 70001 with C = 64 needs more blocks than the grid cap (16384).
    sel None: every row in place; sel with -1 entries: those rows are dropped, the others go to their slots"""
    rng = np.random.RandomState(M + C)
    pts = (rng.randn(M, 3 + C) * 10).astype(np.float32)
    offset = (0.1, -2.3, 7.7)
    d_pts = _dev(pts, device)
    for masked in (False, True):
        mask = (rng.rand(M) < 0.6) if masked else None
        if masked and M > 1:
            mask[0], mask[-1] = False, True
        n_out = int(mask.sum()) if masked else M
        sel = None
        if masked:
            sel = _dev(np.where(mask, np.cumsum(mask) - 1, -1).astype(np.int32), device)
        coords = torch.full((n_out * 3 + 16,), float(CANARY), dtype=torch.float32, device=device)
        feats = torch.full((n_out * C + 16,), float(CANARY), dtype=torch.float32, device=device)
        _call("cnrma_select_rows_f32", d_pts.data_ptr(), M, C, sel.data_ptr() if masked else None, *offset, coords.data_ptr(),
              feats.data_ptr(), _stream())
        ec, ef = O.select_rows(torch.from_numpy(pts), offset, mask)
        gc, gf = coords.cpu().numpy(), feats.cpu().numpy()
        assert (gc[n_out * 3:] == CANARY).all() and (gf[n_out * C:] == CANARY).all()
        assert np.array_equal(gc[:n_out * 3].view(np.uint32), ec.numpy().reshape(-1).view(np.uint32)), (M, C, masked)
        assert np.array_equal(gf[:n_out * C].view(np.uint32), ef.numpy().reshape(-1).view(np.uint32)), (M, C, masked)
