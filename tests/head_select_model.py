"""The selection rule of the FCAF3D head, restated plainly in numpy / float64, and builders for inputs on which it is decided
without doubt (tests/test_head_select_cpu.py, tests/test_head_select_gpu.py).

The rule.  Rows come scene-major.  Rows of one scene are ranked by descending score; rows of equal score by ascending row index.
  pruning:  a scene keeps its min(n_b, T) best rows; the kept rows of all scenes stay in row order.
  cut:      a scene with more than nms_pre > 0 rows on a level gives its nms_pre best rows, best first; every other scene (and
            every scene when nms_pre <= 0) gives all its rows in row order.

The builders make score fields of a few hundred distinct values whose neighbours differ by at least GAP = 1e-3 -- a thousand times
the 1e-6 to which the device's sigmoid product is pinned -- so that a float32 ranking and a float64 ranking can only differ inside a
group of rows that were given the same value on purpose; such rows get bit-identical logits."""
import numpy as np

GAP = 1e-3
PALETTE = 990                # distinct ordinary score values: 0.004 + m * 1.001e-3, m < PALETTE (the largest is 0.99399)
ZERO, ONE = -1, 1000         # group keys of the two saturated values: score exactly +0.0 and exactly 1.0 (keys order like scores)
PATTERNS = ("plain", "straddle5", "zeros", "ones", "equal")


# ---------------------------------------------------------------------------------------------------------------------
# the rule
# ---------------------------------------------------------------------------------------------------------------------
def ranked(rows, scores):
    """`rows` by descending score, equal scores by ascending row index"""
    rows = np.sort(np.asarray(rows, dtype=np.int64))
    return rows[np.lexsort((rows, -np.asarray(scores, dtype=np.float64)[rows]))]


def _n_scenes(scene_ids, n_scenes):
    return int(n_scenes) if n_scenes is not None else (int(np.max(scene_ids)) + 1 if len(scene_ids) else 1)


def prune_rows(scene_ids, interp_scores, T, n_scenes=None):
    """row indices kept by the pruning step, ascending (T < 0: pruning is off, every row stays)"""
    scene_ids = np.asarray(scene_ids, dtype=np.int64).reshape(-1)
    scores = np.asarray(interp_scores, dtype=np.float64).reshape(-1)
    kept = []
    for b in range(_n_scenes(scene_ids, n_scenes)):
        rows = np.nonzero(scene_ids == b)[0]
        kept.append(rows if T < 0 or len(rows) <= T else ranked(rows, scores)[:T])
    return np.sort(np.concatenate(kept)).astype(np.int64)


def cut_rows(scene_ids, max_scores, nms_pre, n_scenes=None):
    """per scene: the row indices that the pre-NMS cut passes on, in the reference's order"""
    scene_ids = np.asarray(scene_ids, dtype=np.int64).reshape(-1)
    scores = np.asarray(max_scores, dtype=np.float64).reshape(-1)
    out = []
    for b in range(_n_scenes(scene_ids, n_scenes)):
        rows = np.nonzero(scene_ids == b)[0].astype(np.int64)
        out.append(ranked(rows, scores)[:nms_pre] if len(rows) > nms_pre > 0 else rows)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# builders: which rows share a value
# ---------------------------------------------------------------------------------------------------------------------
def _chunks(count, t):
    return [t] * (count // t) + ([count % t] if count % t else [])


def scene_groups(n, k, pattern, rng):
    """group key per row of one scene of n rows, for a cut at k.  Rows of one key tie; a larger key is a larger score.
    plain:      as many distinct values as the palette gives (no ties up to PALETTE rows, runs of equal rank-neighbours above)
    straddle5:  the rows of rank k-3 .. k+1 (three inside the cut, two outside) share one value          (needs n >= k + 2)
    zeros:      the rows from rank k-2 to the last are exactly +0.0: the block begins inside the cut and reaches past it
    ones:       the k + 2 best rows are exactly 1.0                                                      (needs n >= k + 2)
    equal:      every row has the same value
    A scene too small for its pattern is plain.  The ranks are dealt to the rows by a random permutation."""
    assert pattern in PATTERNS
    if pattern in ("straddle5", "ones") and not (n >= k + 2 and k >= 3):
        pattern = "plain"
    if pattern == "zeros" and not (n > k >= 2):
        pattern = "plain"
    t = max(1, -(-n // (PALETTE - 3)))
    if pattern == "plain":
        sizes, special = _chunks(n, t), {}
    elif pattern == "straddle5":
        head = _chunks(k - 3, t)
        sizes, special = head + [5] + _chunks(n - k - 2, t), {}
    elif pattern == "zeros":
        head = _chunks(k - 2, t)
        sizes, special = head + [n - k + 2], {len(head): ZERO}
    elif pattern == "ones":
        sizes, special = [k + 2] + _chunks(n - k - 2, t), {0: ONE}
    else:
        sizes, special = ([n] if n else []), {}
    step = max(1, PALETTE // max(len(sizes), 1))
    by_rank = np.concatenate([np.full(s, special.get(g, PALETTE - 1 - g * step), dtype=np.int64) for g, s in enumerate(sizes)]
                             + [np.zeros(0, dtype=np.int64)])
    assert len(by_rank) == n and (n == 0 or by_rank.min() >= ZERO)
    keys = np.empty(n, dtype=np.int64)
    keys[rng.permutation(n)] = by_rank
    return keys


def level_groups(counts, k, pattern, seed):
    """(scene id per row, group key per row) of one scene-major row set with counts[b] rows of scene b"""
    rng = np.random.RandomState(seed)
    scene = np.concatenate([np.full(n, b, dtype=np.int64) for b, n in enumerate(counts)] + [np.zeros(0, dtype=np.int64)])
    keys = np.concatenate([scene_groups(n, k, pattern, rng) for n in counts] + [np.zeros(0, dtype=np.int64)])
    return scene, keys


# ---------------------------------------------------------------------------------------------------------------------
# builders: head logits whose max class score x centerness takes the group's value
# ---------------------------------------------------------------------------------------------------------------------
def sigmoid64(x):
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-np.asarray(x, dtype=np.float64)))


def group_logits(key, n_cls):
    """float32 [1 + n_cls]: centerness logit, class logits.  A function of the key alone, so rows of one key are bit-identical."""
    row = np.empty(1 + n_cls, dtype=np.float32)
    if key == ZERO:
        row[0], row[1:] = 0.3, -200.0                      # sigmoid(-200) is below the smallest float32: the product is +0.0
    elif key == ONE:
        row[0], row[1:] = 200.0, -3.0                      # sigmoid(200) rounds to 1.0 in float32 and in float64
        row[1] = 200.0
    else:
        s = 0.004 + key * 1.001e-3
        row[0] = 20.0 if (key % 2 == 0 or s >= 0.7) else 1.0
        p = s / sigmoid64(row[0])                           # the class probability that gives the score s
        top = np.float32(np.log(p / (1.0 - p)))
        col = key % n_cls
        row[1:] = [top - np.float32(1.0 + 0.25 * ((j - col) % n_cls)) for j in range(n_cls)]
        row[1 + col] = top
    return row


def head_logits(keys, n_cls):
    """(centerness [n, 1], cls_score [n, n_cls]) float32 of the rows with these group keys"""
    table = {int(g): group_logits(int(g), n_cls) for g in np.unique(keys)}
    rows = np.stack([table[int(g)] for g in keys]) if len(keys) else np.zeros((0, 1 + n_cls), dtype=np.float32)
    return np.ascontiguousarray(rows[:, :1]), np.ascontiguousarray(rows[:, 1:])


def class_scores64(cls_score, centerness):
    """sigmoid(cls) * sigmoid(centerness) in float64, from the float32 logits"""
    return sigmoid64(cls_score) * sigmoid64(np.asarray(centerness).reshape(-1, 1))


def cut_level(counts, k, pattern, n_cls, seed):
    """one level of head outputs: dict(scene, keys, cen [n,1], cls [n,n_cls], score = float64 max class score x centerness)"""
    scene, keys = level_groups(counts, k, pattern, seed)
    cen, cls = head_logits(keys, n_cls)
    score = class_scores64(cls, cen).max(axis=1) if len(keys) else np.zeros(0)
    return dict(scene=scene, keys=keys, cen=cen, cls=cls, score=score, counts=tuple(counts))


def identity_rows(n, n_reg):
    """points[i] = (i, 0, 0) and a bbox_pred of equal opposite distances: the decoded box centre is the point, box[:, 0] == i
    exactly (i < 2**24) in every yaw mode; the two yaw outputs are non-zero (their norm divides)"""
    pts = np.zeros((n, 3), dtype=np.float32)
    pts[:, 0] = np.arange(n)
    box = np.ones((n, n_reg), dtype=np.float32)
    if n_reg > 6:
        box[:, 6:] = (0.3, 0.4, 0.5)[:n_reg - 6]
    return pts, box


# ---------------------------------------------------------------------------------------------------------------------
# builders: pruning inputs
# ---------------------------------------------------------------------------------------------------------------------
def prune_value(keys):
    """float32 score of a group key for the pruning tests (raw class logits: any float).  Dyadic, so that every weighted sum of an
    interpolation is exact in float32 in any order: +0.0 for ZERO, (m + 1) / 512 for the palette, 2.0 -- the largest -- for ONE"""
    keys = np.asarray(keys, dtype=np.int64)
    return np.where(keys == ZERO, 0.0, np.where(keys == ONE, 2.0, (keys + 1) / 512.0)).astype(np.float32)


def site(i, pitch):
    """a lattice site per row index: a 32 x 32 x n block of pitch `pitch`"""
    i = np.asarray(i, dtype=np.int64)
    return np.stack((i % 32, (i // 32) % 32, i // 1024), axis=1) * pitch


def prune_level(counts, T, pattern, stride, seed, off_site=False):
    """inputs of FCAF3DHead._prune: x at tensor stride `stride` (coordinates [n, 4], scene-major, features [n, 3] that name the
    row) and the coarser level's scores (coordinates [m, 4], values [m, 1]) on the lattice of 2 * stride.
    on-site:   every query is a coarse site that holds its group's value: the interpolation returns it exactly.
    off-site:  row j of a scene sits half a coarse cell off its site a in x (even j) or in x and y (odd j).  The site holds twice
               (four times) the group's value; the other corner in x is missing for even j and holds zero for odd j, the corners
               in y are missing: the interpolated value is the group's value again, through weights of 1/2 and 1/4."""
    scene, keys = level_groups(counts, T, pattern, seed)
    n, s = len(keys), stride
    val = prune_value(keys)
    j = np.concatenate([np.arange(c) for c in counts] + [np.zeros(0, dtype=np.int64)]).astype(np.int64)
    feats = np.stack((np.arange(n), scene, keys), axis=1).astype(np.float32)
    if not off_site:
        xyz = site(j, 2 * s)
        coords = np.concatenate((scene[:, None], xyz), axis=1)
        return dict(scene=scene, keys=keys, coords=coords, feats=feats, score_coords=coords.copy(), score=val.reshape(-1, 1),
                    value=val.astype(np.float64), counts=tuple(counts))
    a = site(j, 4 * s)                                      # one site per row, every second coarse site: no row shares a corner
    odd = (j % 2 == 1)
    q = a.copy()
    q[:, 0] += s
    q[odd, 1] += s
    coords = np.concatenate((scene[:, None], q), axis=1)
    far = a[odd].copy()
    far[:, 0] += 2 * s                                       # the other corner in x of the odd rows: present, value zero
    sc = np.concatenate((np.concatenate((scene[:, None], a), axis=1), np.concatenate((scene[odd][:, None], far), axis=1)))
    sv = np.concatenate((val * np.where(odd, 4.0, 2.0).astype(np.float32), np.zeros(int(odd.sum()), dtype=np.float32)))
    order = np.lexsort((sc[:, 3], sc[:, 2], sc[:, 1], sc[:, 0]))             # scene-major like every row set
    return dict(scene=scene, keys=keys, coords=coords, feats=feats, score_coords=sc[order], score=sv[order].reshape(-1, 1),
                value=val.astype(np.float64), counts=tuple(counts))
