"""ORACLE (test infrastructure only): exact host models of the small kernels around the big ones -- the hashed random
subset and the radix top-k select of csrc/util.hip, the per-ray record selection built on them, and the suppression
matrix of csrc/nms.hip.  Plain numpy; every model is a few lines and is checked on its own in
tests/test_util_oracle_cpu.py.  The scans, the fp64 sum, the layout pass, the range check and the byte fill need no
model beyond numpy itself (cumsum in int64, an integer sum, a transpose, a comparison, a constant)."""
import functools

import numpy as np

from . import post_oracle as PO

_M32 = np.uint64(0xFFFFFFFF)


def _u64(x):
    return np.asarray(x, dtype=np.uint64) & _M32


# ---------------------------------------------------------------------------------------------------------------------
# the sampler: every row gets the 32-bit hash of (seed, row); the n_keep smallest hashes are kept
# ---------------------------------------------------------------------------------------------------------------------
def row_hash(seed, i):
    """row_hash of util.hip in uint32 arithmetic (held in uint64 and masked, so that nothing depends on numpy's overflow
    rules).  Odd multipliers and xor-shifts only: a bijection of i for a fixed seed."""
    x = (_u64(i) * np.uint64(0x9E3779B1) + _u64(seed)) & _M32
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7FEB352D)) & _M32
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846CA68B)) & _M32
    x ^= x >> np.uint64(16)
    return x.astype(np.uint32)


def select_seed(seed, word):
    """the seed a select uses when a device word is mixed in: seed + 0x9E3779B9 * word mod 2^32"""
    return (int(seed) + 0x9E3779B9 * int(word)) & 0xFFFFFFFF


def sample_mask(cap, live, n_keep, seed, word=None):
    """uint8 [cap]: ones at the min(live, n_keep) rows with the smallest hash among the first min(live, cap) rows, zeros
    elsewhere.  The hash has no ties (bijection), so the set is unique."""
    if word is not None:
        seed = select_seed(seed, word)
    live = max(0, min(int(live), int(cap)))
    mask = np.zeros(int(cap), dtype=np.uint8)
    k = min(live, int(n_keep))
    if k > 0:
        h = row_hash(seed, np.arange(live, dtype=np.uint64))
        mask[np.argsort(h, kind="stable")[:k]] = 1
    return mask


# ---------------------------------------------------------------------------------------------------------------------
# the score select: rows ordered by an inverted order-preserving key of the float's bit pattern
# ---------------------------------------------------------------------------------------------------------------------
def select_key(score_bits):
    """uint32 key of a float32 bit pattern: ascending key = descending score in IEEE total order (sign-magnitude bits:
    -0.0 below +0.0, a NaN with a clear sign bit above +inf, one with a set sign bit below -inf)"""
    u = np.asarray(score_bits, dtype=np.uint32)
    ordered = np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000))
    return (~ordered).astype(np.uint32)


def scores_from_keys(keys):
    """inverse of select_key: the float32 values (any bit pattern, NaNs included) whose keys are `keys`"""
    k = np.asarray(keys, dtype=np.uint32)
    u = np.where(k & np.uint32(0x80000000), k, (~k) & np.uint32(0x7FFFFFFF)).astype(np.uint32)
    return u.view(np.float32)


def score_bits(scores):
    return np.ascontiguousarray(np.asarray(scores, dtype=np.float32)).view(np.uint32)


def topk_rows(scores, live, k):
    """int64 rows of the k best scores among the first `live`, sorted by (key ascending, row ascending), cut at
    min(live, k): the order cnrma_topk_indices_f32 states; as a set, the ones of cnrma_topk_mask_f32"""
    live = max(0, min(int(live), len(scores)))
    keys = select_key(score_bits(scores)[:live])
    return np.argsort(keys, kind="stable")[:min(live, int(k))].astype(np.int64)


def key_digits(key):
    """the three radix digits of a key: bits 31..21, 20..10, 9..0"""
    key = int(key)
    return key >> 21, (key >> 10) & 2047, key & 1023


# ---------------------------------------------------------------------------------------------------------------------
# the sampler applied to the march's per-ray sample records
# ---------------------------------------------------------------------------------------------------------------------
def select_records(row_offset, kept, cap, live, n_keep, seed, word=None):
    """int32 [n, 4]: the kept rows of sample_mask(cap, live, n_keep, seed, word) in row order, each as
    (ray, kept[ray][row - off[ray]].y, .x, 0).  Ray r owns rows [off[r], min(off[r + 1], live)); kept is int32
    [R, slots, 2] = (x, y) per slot."""
    off = np.asarray(row_offset, dtype=np.int64)
    kept = np.asarray(kept)
    live = max(0, min(int(live), int(cap)))
    rows = np.nonzero(sample_mask(cap, live, n_keep, seed, word))[0]
    ray = np.searchsorted(np.minimum(off[1:], live), rows, side="right")
    slot = rows - off[ray]
    rec = np.zeros((len(rows), 4), dtype=np.int32)
    rec[:, 0] = ray
    rec[:, 1] = kept[ray, slot, 1]
    rec[:, 2] = kept[ray, slot, 0]
    return rec


# ---------------------------------------------------------------------------------------------------------------------
# NMS: the suppression matrix, and how far the inputs of a test stay from the threshold
# ---------------------------------------------------------------------------------------------------------------------
def nms_boxes(n, rotated, seed):
    """float32 [n, 7] boxes in score order for the mask tests: centres in a 2.5 m cube, sizes 0.3 .. 1.5 m, any yaw"""
    rng = np.random.RandomState(seed)
    b = np.zeros((n, 7), dtype=np.float32)
    b[:, :3] = rng.rand(n, 3) * 2.5
    b[:, 3:6] = 0.3 + rng.rand(n, 3) * 1.2
    if rotated:
        b[:, 6] = rng.uniform(-3.2, 3.2, n)
    return b


# the mask tests: box counts around the 64-bit word boundaries, both box kinds, three thresholds; the seed of a kind is the
# first whose 129 boxes keep every pairwise IoU at least NMS_MARGIN from every threshold (seeds 0..7 come closer than that to
# 0.1; test_util_oracle_cpu.py asserts the margin for every case)
NMS_COUNTS = (1, 2, 63, 64, 65, 128, 129)
NMS_THRESHOLDS = (0.1, 0.3, 0.5)
NMS_MARGIN = 1e-4          # 5 x the 2e-5 by which the float32 IoU may differ from the oracle
NMS_SEEDS = {True: 8, False: 8}     # rotated: margins 2.1e-4 / 2.3e-4 / 1.3e-3; axis-aligned: 1.1e-4 / 5.4e-4 / 4.5e-4


def pair_iou(boxes):
    """float64 [n, n], upper triangle: BEV IoU of the clipping oracle for every pair i < j (zeros elsewhere)"""
    n = len(boxes)
    out = np.zeros((n, n), dtype=np.float64)
    for i in range(n):
        for j in range(i + 1, n):
            out[i, j] = PO.iou(boxes[i], boxes[j], mode3d=False)
    return out


@functools.lru_cache(maxsize=None)
def _largest_case(rotated):
    full = nms_boxes(max(NMS_COUNTS), rotated, NMS_SEEDS[rotated])
    return full, pair_iou(full)


def nms_case(n, rotated):
    """(boxes, pair_iou) of one mask test: the first n boxes of the largest set of their kind, whose oracle matrix is
    computed once and serves every count"""
    full, iou = _largest_case(bool(rotated))
    return full[:n], iou[:n, :n]


def suppression_bits(boxes, thr, iou=None):
    """uint64 [n, ceil(n / 64)]: bit j of row i set where j > i and oracle IoU(i, j) > thr (iou: pair_iou(boxes), when the
    caller has it)"""
    n = len(boxes)
    hit = np.triu((pair_iou(boxes) if iou is None else iou) > thr, 1)
    words = (n + 63) // 64
    out = np.zeros((n, words), dtype=np.uint64)
    for w in range(words):
        blk = hit[:, 64 * w:64 * w + 64]
        out[:, w] = (blk.astype(np.uint64) << np.arange(blk.shape[1], dtype=np.uint64)[None, :]).sum(axis=1, dtype=np.uint64)
    return out


def min_threshold_margin(boxes, thr, iou=None):
    """smallest |IoU(i, j) - thr| over all pairs i < j (inf for a single box)"""
    n = len(boxes)
    if n < 2:
        return float("inf")
    return float(np.abs((pair_iou(boxes) if iou is None else iou)[np.triu_indices(n, 1)] - thr).min())


def greedy_keep(bits):
    """the greedy pass over a suppression matrix: rows kept in order"""
    n, words = bits.shape
    removed = np.zeros(words, dtype=np.uint64)
    keep = []
    for i in range(n):
        if not (removed[i >> 6] >> np.uint64(i & 63)) & np.uint64(1):
            keep.append(i)
            removed |= bits[i]
    return np.array(keep, dtype=np.int64)
