"""GPU tests (-m gpu) of the sparse convolutions and their companions at edge shapes, widths and live counts, against the fp64
oracle (oracle/sparse_oracle.py), through cnrma_amd.sparse and the PRODUCT library only (conv_tuning() is never called).

tests/test_sparse_gpu.py drives every family with a few thousand random rows, channel widths that are multiples of 32 / 64
and sets whose capacity equals their row count.  Here the same kernels meet what the launchers can be handed and nothing ran:

  A  test_edge_matrix / test_generative_transpose_edges / test_gather_once_bf16_edges: every family (stage fp32, stage on a
     prepared image, gather-once, pair list, generative transpose; the C entry that ran is asserted) at 1 / 2 / 63 / 64 / 65 /
     129 rows, Cin 32 / 96 / 160 (512: the test_cin512_* tests, every family; 1 / 31 / 33 on the fp32 fallback), the column tails of every family, isolated rows, a dense
     block in random row order, two scenes with the same xyz, negative coordinates under stride 2 and 4, a strided
     convolution with one output row, and every epilogue on a launch that splits and on one that does not.
  B  test_capacity_*: a capacity larger than the live count with the dead rows poisoned (coordinates that would be duplicates
     and false neighbours, features 3e38 or NaN): live rows equal the oracle on the live rows alone and -- where the plan is
     the same -- the exact-size run bit for bit; magnitude bounds, statistics and counts are those of the live rows; tables
     never name a dead row.  The eager wrappers size derived sets from a count they read back, so the OUTPUT side gets its
     capacity the way a static trace gives it: strided_with_capacity() (strided convolutions, the pair list, pooling, the
     strided tables) and the C entries of union_add / prune called with out_cap and a device count (test_capacity_ops).
  C  test_every_product_launcher_choice_has_a_case + test_stage_launcher_choice / test_gather_once_launcher_choice: the two
     planners enumerated over a grid that crosses every threshold, every distinct result run against the oracle with the
     full epilogue (the capacity reaches the large-row branches with a few hundred live rows).

Where the items of the issue live:
  1 odd numbers of 32-channel slices .......... test_gather_once_uneven_last_split, test_cin512_* (every family),
                                                test_gather_once_launcher_choice (uneven ids), test_edge_matrix[go-*-c96|c160-*]
  2 column tails .............................. test_edge_matrix[go-*-o65|o66|o72|o96|o160|o200], [pairs-*-o4|o36|o68],
                                                [stage-*-o1|o3|o33]
  3 row counts around a tile .................. test_edge_matrix[*-rows1 .. rows129], test_auto_switch_between_stage_and_gather_once
  4 degenerate kernel maps .................... test_edge_matrix[*-lattice|twin|one_out|neg*], test_stage_split_with_empty_offset_groups
  5 the live-count contract ................... test_capacity_conv, test_capacity_generative_transpose, test_capacity_ops,
                                                test_capacity_tables, test_live_zero
  6 the product launcher's branches ........... section C
  7 the 16-bit coordinate key ................. test_no_neighbour_across_the_key_wrap (exposed a false neighbour; fixed by
                                                hash_find_site() in csrc/common.h: probes outside the key range find nothing)

Bars: fp32-grade paths 2e-6 of max(1, max|oracle|) up to a dot length of 27 x 256 (the suite's bound); Cin = 512: the
sum|a||b| bounds of test_bf16x6_is_fp32_grade_on_wide_dynamic_range (see test_cin512_error_against_sum_abs); bf16 entries
1e-5 against fp64 accumulation of bf16-rounded operands (tests/test_train_gpu.py); every index output exact; f16x3 magnitude
bound == max|out| over the live rows; every case twice, bit-identical."""
import contextlib
import itertools

import numpy as np
import pytest
import torch

from helpers import POISON, capacity_tensor, poison_coords, poison_rows
from oracle import sparse_oracle as SO

pytestmark = pytest.mark.gpu
TOL = 2e-6
LONG_DOT = 27 * 256          # the suite's 2e-6 bound is established up to this dot length

CONV_ENTRIES = {"cnrma_sparse_conv_f32", "cnrma_sparse_conv_f16x3", "cnrma_sparse_conv_bf16x6", "cnrma_sparse_conv_bf16",
                "cnrma_sparse_conv_go_f16x3", "cnrma_sparse_conv_go_f32", "cnrma_sparse_conv_go_bf16",
                "cnrma_sparse_conv_pairs_f16x3", "cnrma_sparse_conv_pairs_f32", "cnrma_sparse_convtr_gen_f16x3",
                "cnrma_sparse_convtr_gen_bf16x6", "cnrma_sparse_convtr_gen_f32"}


# ---------------------------------------------------------------------------------------------------------------------
# plumbing
# ---------------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def recorded_calls():
    """names of the C-ABI entries cnrma_amd.sparse calls inside the block"""
    from cnrma_amd import sparse as S
    seen, orig = [], S.call

    def call(name, *a):
        seen.append(name)
        return orig(name, *a)
    S.call = call
    try:
        yield seen
    finally:
        S.call = orig


@contextlib.contextmanager
def settings(**kw):
    """module switches of cnrma_amd.sparse (GO_CONV, PAIR_CONV, ...: product settings, not conv_tuning) for the block"""
    from cnrma_amd import _lib
    from cnrma_amd import sparse as S
    assert not _lib.experiments_active()
    prev = {k: getattr(S, k) for k in kw}
    for k, v in kw.items():
        setattr(S, k, v)
    try:
        yield
    finally:
        for k, v in prev.items():
            setattr(S, k, v)


FAMILY_SETTINGS = {"stage": dict(GO_CONV=False, PAIR_CONV=False), "go": dict(GO_CONV=True, PAIR_CONV=False),
                   "auto": dict(GO_CONV="auto", PAIR_CONV=False),
                   "pairs": dict(GO_CONV=False, PAIR_CONV=True, PAIR_CONV_MIN_CIN=32)}
FAMILY_SETTINGS["stage2"] = FAMILY_SETTINGS["stage"]          # the stage kernel under stride 2


def bf16_round(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(torch.bfloat16).float().numpy()


def block(n, ts=1, seed=0, lo=0, batch=0):
    """n voxels of a dense cube in random row order (no locality: tiles need several offset groups) at tensor stride ts;
    lo: the cube's lowest voxel (negative: negative coordinates, odd multiples of ts included)"""
    side = 1
    while side ** 3 < n:
        side += 1
    g = np.stack(np.meshgrid(*[np.arange(side)] * 3, indexing="ij"), axis=-1).reshape(-1, 3)
    g = g[np.random.RandomState(1000 * seed + n).permutation(len(g))[:n]]
    return np.concatenate((np.full((n, 1), batch), (g + lo) * ts), axis=1).astype(np.int64)


def lattice(n, ts=1, step=3):
    """n isolated voxels: a lattice of every third site, so only the centre offset has a neighbour and a stride-2 coarsening
    merges nothing (the pair list's sparse sample)"""
    side = 1
    while side ** 3 < n:
        side += 1
    g = np.stack(np.meshgrid(*[np.arange(side)] * 3, indexing="ij"), axis=-1).reshape(-1, 3)[:n]
    return np.concatenate((np.zeros((n, 1), dtype=np.int64), (g - side // 2) * step * ts), axis=1).astype(np.int64)


def twin(c):
    """two scenes with identical xyz, rows interleaved"""
    c2 = np.repeat(c, 2, axis=0)
    c2[1::2, 0] = 1
    return c2


GEOMETRY = {
    "rows1": lambda ts: block(1, ts), "rows2": lambda ts: block(2, ts, lo=-1), "rows63": lambda ts: block(63, ts, lo=-2),
    "rows64": lambda ts: block(64, ts), "rows65": lambda ts: block(65, ts, lo=-3), "rows129": lambda ts: block(129, ts, lo=-2),
    "block": lambda ts: block(300, ts, lo=-4), "lattice": lambda ts: lattice(200, ts), "twin": lambda ts: twin(block(150, ts, lo=-2)),
    "neg": lambda ts: block(300, ts, lo=-11),                              # every coordinate negative
    "one_out": lambda ts: block(8, ts)[:5],                                # 5 of the 8 voxels of one coarse cell
    "sparse1": lambda ts: lattice(1, ts), "sparse2": lambda ts: lattice(2, ts), "sparse63": lambda ts: lattice(63, ts),
    "sparse64": lambda ts: lattice(64, ts), "sparse65": lambda ts: lattice(65, ts), "sparse129": lambda ts: lattice(129, ts),
    "sparse_twin": lambda ts: twin(lattice(100, ts)), "sparse_neg": lambda ts: lattice(150, ts) - np.array([0, 40, 40, 40]) * ts,
}


def epilogue(kind, seed, live, cap, cout, device):
    """kind: none | ss (scale + shift) | relu | elu (scale + shift + residual + activation) -> (conv() keywords, fp64 reference)"""
    if kind == "none":
        return {}, lambda y: y
    rng = np.random.RandomState(seed + 77)
    scale = (0.5 + rng.rand(cout)).astype(np.float32)
    shift = (0.3 * rng.randn(cout)).astype(np.float32)
    kw = dict(scale=torch.from_numpy(scale).to(device), shift=torch.from_numpy(shift).to(device))
    res = None
    if kind in ("relu", "elu"):
        res = rng.randn(live, cout).astype(np.float32)
        kw.update(residual=poison_rows(res, cap, device), act=kind)
    elif kind.startswith("ss+"):                                    # the generative transpose has no residual
        kw.update(act=kind[3:])

    def ref(y):
        y = y * scale.astype(np.float64) + shift.astype(np.float64)
        if res is not None:
            y = y + res.astype(np.float64)
        act = kw.get("act")
        return SO.relu(y) if act == "relu" else (SO.elu(y) if act == "elu" else y)
    return kw, ref


def sum_abs(c, f, W, ks, stride, ts):
    """sum |a||b| of every output's dot product (fp64): the natural scale of its rounding error"""
    return SO.conv(c, np.abs(f), np.abs(W), ks, stride, ts)[1]


def close(got, exp, bf16=False, mag=None, mag_bound=None, gain=1.0):
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == exp.shape and np.isfinite(got).all()
    if bf16:                                                        # tests/test_train_gpu.py: fp32 accumulation of bf16 operands
        np.testing.assert_allclose(got, exp, rtol=1e-5, atol=1e-5)
    elif mag is not None:
        # a dot product longer than the 2e-6 bound is established for: its error against sum|a||b| (the bound of
        # test_bf16x6_is_fp32_grade_on_wide_dynamic_range), carried through the epilogue -- times the largest scale, plus one fp32
        # rounding (2^-24 relative) for each of its three operations and the activation
        err = np.abs(got - exp).max()
        bar = mag_bound * mag.max() * gain + 4 * 2.0 ** -24 * max(1.0, float(np.abs(exp).max()))
        print("max error %.3e, %.3e of the largest sum|a||b| (bar %.1e)" % (err, err / mag.max(), mag_bound))
        assert err <= bar, (err, bar)
    else:
        np.testing.assert_allclose(got, exp, rtol=TOL, atol=TOL * max(1.0, float(np.abs(exp).max())))


def stage_key(prec, cap, cin, cout, K, slices=1):
    from cnrma_amd import sparse as S
    p = S.conv_plan(cap, cin, cout, K, prec, slices)
    return (prec if cin % 32 == 0 else "f32", p["shape"], p["splits"] > 1, p["prefetch"])


def go_key(cap, cin, cout, residual):
    from cnrma_amd import sparse as S
    p = S.conv_go_plan(cap, cin, cout, residual)
    uneven = p["splits"] > 1 and (cin // 32) % p["slices_per_split"] != 0
    return (p["columns"], p["splits"] > 1, uneven, p["order"], p["residual_in_kernel"])


def strided_with_capacity(cs, out_cap, by_sort=False):
    """the stride-2 output set of `cs` with a CAPACITY and a device live word: what CoordSet.prefetch_strided builds inside a
    static trace, made by hand through the same C entries (cnrma_sparse_stride_coords / _sorted with out_cap > 0) -- the eager
    wrapper reads the count back and returns an exact-size set, so no kernel behind it ever sees no_cap > live.  The dead rows of
    the output hold plausible poison (coordinates of the input); the set is cached on `cs`, so conv / max_pool /
    instance_norm_max_pool / neighbours pick it up"""
    from cnrma_amd import _lib
    from cnrma_amd import sparse as S
    assert out_cap <= cs.n
    ns, dev = 2 * cs.stride, cs.device
    ws = torch.empty(_lib.load().cnrma_voxelize_workspace_bytes(cs.n), dtype=torch.uint8, device=dev)
    out = cs.C.clone()
    n_out = torch.empty(1, dtype=torch.int32, device=dev)
    if by_sort:
        m = None
        S.call("cnrma_sparse_stride_coords_sorted", S.ptr(cs.C), cs.n, S.ptr(cs.n_dev), ns, S.ptr(out), out_cap, S.ptr(n_out), S.ptr(ws),
               S.stream())
    else:
        m = S.CoordMap(out_cap, dev)
        S.call("cnrma_sparse_stride_coords", S.ptr(cs.C), cs.n, S.ptr(cs.n_dev), ns, S.ptr(m.keys), S.ptr(m.vals), m.cap, S.ptr(out),
               out_cap, S.ptr(n_out), S.ptr(ws), S.stream())
    child = S.CoordSet(out, ns, m, cs.n_batch, n=out_cap, n_dev=n_out)
    child.scene_major, child.compact, child.sorted = cs.scene_major, cs.compact, cs.sorted
    cs._children[ns] = child
    return child


def run_conv(device, c, f, W, family, precision, ks=3, stride=1, ts=1, epi="none", cap=None, value=POISON, compact=False,
             seed=0, split=None, entry=None, out_cap=None):
    """S.conv on (c, f) under the family's settings, twice on freshly built sets: asserts the entry that ran, run-to-run bit
    identity, exact output coordinates, the oracle's values on the live rows (bf16: on bf16-rounded operands), the f16x3
    magnitude bound, and `split` (whether the launch splits) where given.  Returns (live output rows, magnitude bound, plan)."""
    from cnrma_amd import sparse as S
    K, cin, cout = W.shape
    live = len(c)
    bf16 = precision == "bf16" and cin % 32 == 0
    fo, Wo = (bf16_round(f), bf16_round(W)) if bf16 else (f, W)
    oc, of = SO.conv(c, fo, Wo, ks, stride, ts)
    cap_in = live if cap is None else cap
    live_out, cap_out = (live, cap_in) if stride == 1 else (len(oc), len(oc) if out_cap is None else out_cap)
    kw, ref = epilogue(epi, seed, live_out, cap_out, cout, device)
    exp = ref(of)
    Wd = torch.from_numpy(W).to(device)
    if entry is None:
        entry = {"stage": "cnrma_sparse_conv_" + (precision if cin % 32 == 0 else "f32"), "go": "cnrma_sparse_conv_go_" + precision,
                 "pairs": "cnrma_sparse_conv_pairs_" + precision, "stage2": "cnrma_sparse_conv_" + precision}[family]
    outs = []
    with settings(**FAMILY_SETTINGS[family]):
        for _ in range(2):
            x = capacity_tensor(c, f, ts, device, cap, value, compact=compact)
            if out_cap is not None:                       # a strided output set with a capacity and a live word of its own
                strided_with_capacity(x.cs, out_cap)
            with recorded_calls() as seen:
                y = S.conv(x, Wd, ks, stride, precision=precision, **kw)
            assert [n for n in seen if n in CONV_ENTRIES] == [entry], seen
            outs.append(y)
    y = outs[0]
    assert y.cs.n == cap_out and y.cs.stride == ts * stride
    if out_cap is not None:
        assert int(y.cs.n_dev[0]) == live_out < out_cap
    assert (y.C[:live_out].cpu().numpy().astype(np.int64) == oc).all()
    got = y.F[:live_out]
    assert torch.equal(got, outs[1].F[:live_out]), "run to run"
    mag = None
    if K * cin > LONG_DOT and not bf16:
        mag = sum_abs(c, f, W, ks, stride, ts)
    close(got.cpu().numpy(), exp, bf16, mag, 8e-7 if precision == "f16x3" else 4e-7,
          float(kw["scale"].abs().max()) if "scale" in kw else 1.0)
    amax = None
    if precision == "f16x3" and cin % 32 == 0:
        amax = float(y.amax.max())
        assert amax == float(got.abs().max()) and amax == float(outs[1].amax.max())
    if entry.startswith("cnrma_sparse_conv_go_"):
        plan = S.conv_go_plan(cap_out, cin, cout, "residual" in kw)
    elif entry.startswith("cnrma_sparse_conv_pairs_"):
        plan = None
    else:
        plan = S.conv_plan(cap_out, cin, cout, K, precision)
    if split is not None:
        assert (plan["splits"] > 1) == split, plan
    return got, amax, plan


def weights(K, cin, cout, seed=0):
    return (np.random.RandomState(seed + 31 * cin + cout).randn(K, cin, cout) / np.sqrt(cin * K)).astype(np.float32)


def features(n, C, seed=0):
    return np.random.RandomState(seed + 7 * n + C).randn(n, C).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------------
# A. the edge matrix
# ---------------------------------------------------------------------------------------------------------------------
def _edge_cases():
    """(family, precision, geometry, cin, cout, stride, ts, epilogue, capacity, splits?) -- not a cross product: every value of
    every axis at least once per family, and the combinations the issue names"""
    cases = []
    rows = ("rows1", "rows2", "rows63", "rows64", "rows65", "rows129")
    # ---- stage kernel: rows x precision, Cin 32 / 96 / 160 and the narrow widths 1 / 3 / 33 with K = 27
    wid = itertools.cycle([(32, 1), (96, 3), (160, 33), (32, 64), (96, 33), (160, 3)])
    for r in rows:
        for prec in ("f32", "f16x3", "bf16x6", "bf16"):
            cin, cout = next(wid)
            cases.append(("stage", prec, r, cin, cout, 1, 1, "none", None, None))
    for cin, cout in ((1, 33), (31, 64), (33, 3)):                            # the fp32 fallback (any precision asked for)
        cases.append(("stage", "f16x3", "rows65", cin, cout, 1, 1, "relu", None, None))
        cases.append(("stage", "f32", "rows129", cin, cout, 2, 1, "ss", None, None))
    for prec in ("f32", "f16x3", "bf16x6", "bf16"):
        for geo, stride, ts in (("lattice", 1, 1), ("twin", 1, 2), ("block", 1, 1), ("neg", 2, 1), ("neg", 2, 2), ("one_out", 2, 1),
                                ("one_out", 2, 2)):
            cases.append(("stage", prec, geo, 32, 33, stride, ts, "elu", None, None))
    for epi in ("none", "ss", "relu", "elu"):                                  # every epilogue, split and not split
        for prec in (("f32", "f16x3", "bf16x6", "bf16") if epi == "relu" else ("f16x3",)):
            cases.append(("stage", prec, "block", 96, 64, 1, 1, epi, None, True))
            cases.append(("stage", prec, "block", 96, 64, 1, 1, epi, 70000, False))     # no workspace from 65 536 rows: no split
    # ---- gather-once: rows, Cin 32 / 96 / 160, the column tails
    wid = itertools.cycle([(32, 64), (96, 65), (160, 66), (32, 72), (96, 96), (160, 160), (96, 200)])
    for r in rows:
        for prec in ("f16x3", "f32"):
            cin, cout = next(wid)
            cases.append(("go", prec, r, cin, cout, 1, 1, "none", None, None))
    for cout in (64, 65, 66, 72, 96, 160, 200):
        for prec in ("f16x3", "f32"):
            cases.append(("go", prec, "block", 96, cout, 1, 1, "relu", None, True))
            cases.append(("go", prec, "block", 32, cout, 1, 1, "elu", None, False))    # one slice: nothing to split
    for prec in ("f16x3", "f32"):
        for geo, ts in (("lattice", 1), ("twin", 1), ("twin", 2), ("neg", 4)):
            cases.append(("go", prec, geo, 160, 72, 1, ts, "relu", None, True))
        for epi in ("none", "ss", "relu", "elu"):
            cases.append(("go", prec, "block", 160, 200, 1, 1, epi, None, True))
            cases.append(("go", prec, "block", 160, 200, 1, 1, epi, 70000, False))     # no workspace from 65 536 rows
    # ---- pair list: stride 2 on a sparse sample, Cout 4 / 36 / 68
    wid = itertools.cycle([(32, 4), (96, 36), (160, 68)])
    for r in ("sparse1", "sparse2", "sparse63", "sparse64", "sparse65", "sparse129", "sparse_twin", "sparse_neg"):
        for prec in ("f16x3", "f32"):
            cin, cout = next(wid)
            cases.append(("pairs", prec, r, cin, cout, 2, 1, "none", None, None))
    for epi in ("ss", "relu", "elu"):
        for prec in ("f16x3", "f32"):
            cin, cout = next(wid)
            cases.append(("pairs", prec, "sparse129", cin, cout, 2, 2 if epi == "elu" else 1, epi, None, None))
    return cases


def _edge_id(case):
    fam, prec, geo, cin, cout, stride, ts, epi, cap, split = case
    return "-".join([fam, prec, geo, "c%d" % cin, "o%d" % cout, "s%dt%d" % (stride, ts), epi] + (["cap%d" % cap] if cap else []) +
                    ([] if split is None else ["split" if split else "nosplit"]))


@pytest.mark.parametrize("case", _edge_cases(), ids=_edge_id)
def test_edge_matrix(device, case):
    fam, prec, geo, cin, cout, stride, ts, epi, cap, split = case
    c = GEOMETRY[geo](ts)
    if geo == "one_out":
        assert len(SO.stride_coords(c, 2 * ts)) == 1
    run_conv(device, c, features(len(c), cin), weights(27, cin, cout), fam, prec, 3, stride, ts, epi, cap, split=split)


@pytest.mark.parametrize("prec", ["f16x3", "f32"])
def test_stage_split_with_empty_offset_groups(device, prec):
    """isolated rows under a split over the 27 offsets: every split but the one that holds the centre offset has no neighbour
    in any tile and still has to write its (zero) slab for the reduction"""
    c = lattice(200)
    _, _, plan = run_conv(device, c, features(200, 64), weights(27, 64, 64), "stage", prec, epi="relu", split=True)
    assert plan["k_per_split"] < 13
    with settings(**FAMILY_SETTINGS["stage"]):
        nbr = capacity_tensor(c, features(200, 64), 1, device).cs
        tab = nbr.neighbours(nbr, 3, 1).cpu().numpy()
    assert (tab[:, 13] == np.arange(200)).all() and (np.delete(tab, 13, axis=1) == -1).all()


@pytest.mark.parametrize("rows", [255, 256, 257])
def test_auto_switch_between_stage_and_gather_once(device, rows):
    """GO_CONV = "auto" on a voxelised (compact, Morton-ordered) set: below GO_MIN_ROWS rows the stage kernel, from it on the
    gather-once kernel -- either side of the switch against the oracle"""
    from cnrma_amd import sparse as S
    pts = block(rows, lo=-3)[:, 1:].astype(np.float32) + 0.5
    st, _ = S.voxelize(torch.from_numpy(pts).to(device), torch.from_numpy(features(rows, 64)).to(device), 1.0)
    assert st.cs.n == rows and st.cs.compact
    c, f = st.C.cpu().numpy().astype(np.int64), st.F.cpu().numpy()
    assert S.GO_MIN_ROWS == 256
    entry = "cnrma_sparse_conv_go_f16x3" if rows >= 256 else "cnrma_sparse_conv_f16x3"
    run_conv(device, c, f, weights(27, 64, 72), "auto", "f16x3", epi="relu", compact=True, entry=entry)
    run_conv(device, c, f, weights(27, 64, 72), "auto", "f32", epi="elu", compact=True,
             entry="cnrma_sparse_conv_go_f32" if rows >= 256 else "cnrma_sparse_conv_f32")


@pytest.mark.parametrize("cin,slices", [(256, (3, 3, 2)), (160, (2, 2, 1)), (96, (1, 1, 1))])
@pytest.mark.parametrize("prec", ["f16x3", "f32"])
def test_gather_once_uneven_last_split(device, prec, cin, slices):
    """the split of the real short layers: 256-383 blocks give 3 splits, whose last one is shorter when Cin / 32 is no multiple
    of 3 -- (3, 3, 2) slices at Cin = 256, (2, 2, 1) at 160; reached with 150 row tiles x 2 column tiles of capacity over 400 live rows"""
    c = block(400, lo=-5)
    _, _, plan = run_conv(device, c, features(400, cin), weights(27, cin, 72), "go", prec, epi="relu", cap=64 * 150, split=True)
    ns = cin // 32
    assert plan["splits"] == 3 and plan["slices_per_split"] == slices[0]
    assert tuple(min(ns, (z + 1) * slices[0]) - z * slices[0] for z in range(3)) == slices


@pytest.mark.parametrize("cap,slices", [(64 * 150, (6, 6, 4)), (64 * 70, (3, 3, 3, 3, 3, 1)), (None, None)])
def test_cin512_error_against_sum_abs(device, cap, slices):
    """Cin = 512 with K = 27 (the widest level of the shipped MinkResNet34) is a dot product twice as long as the suite's 2e-6
    bound was ever checked for.  On the same inputs every fp32-grade path is held to the error bounds of
    test_bf16x6_is_fp32_grade_on_wide_dynamic_range against the fp64 oracle: max error <= 4e-7 of the largest sum|a||b| for f32 and
    bf16x6, 8e-7 for f16x3 -- the stage kernels, and the gather-once kernels on their uneven splits (6, 6, 4) and
    (3, 3, 3, 3, 3, 1).  Achieved on MI355X (error / largest sum|a||b|; close() prints them): stage f32 2.8e-8, bf16x6 2.5e-8,
    f16x3 2.1e-8; gather-once (6, 6, 4) f32 6.2e-8, f16x3 5.1e-8; (3, 3, 3, 3, 3, 1) f32 4.5e-8, f16x3 2.8e-8 -- the existing bounds
    hold, so they are asserted unchanged."""
    c = block(320, lo=-4)
    f, W = features(320, 512), weights(27, 512, 72)
    if cap is None:
        for prec in ("f32", "bf16x6", "f16x3"):
            run_conv(device, c, f, W, "stage", prec, epi="relu")
        return
    for prec in ("f32", "f16x3"):
        _, _, plan = run_conv(device, c, f, W, "go", prec, epi="relu", cap=cap, split=True)
        assert plan["splits"] == len(slices) and plan["slices_per_split"] == slices[0]
        assert tuple(min(16, (z + 1) * slices[0]) - z * slices[0] for z in range(len(slices))) == slices


@pytest.mark.parametrize("prec", ["f16x3", "f32"])
def test_cin512_pair_list(device, prec):
    """the pair list at the widest level (its product threshold is Cin >= 128): 27 x 512 products per output at most, held to the
    sum|a||b| bounds of test_cin512_error_against_sum_abs (run_conv switches to them above a dot length of 27 x 256), with the
    full epilogue, once on exact-size sets and once with input and output capacities"""
    c = lattice(129)
    f, W = features(129, 512), weights(27, 512, 68)
    run_conv(device, c, f, W, "pairs", prec, stride=2, epi="relu")
    run_conv(device, c, f, W, "pairs", prec, stride=2, epi="elu", cap=160, out_cap=160)


@pytest.mark.parametrize("prec", ["f16x3", "bf16x6", "f32"])
def test_cin512_generative_transpose(device, prec):
    """the generative transpose at Cin = 512: a dot length of 512 (one weight slice per child), inside the suite's 2e-6 bound"""
    c = block(129, 2, lo=-3)
    run_convtr(device, c, features(129, 512), weights(8, 512, 72), 2, prec, "ss+elu")
    run_convtr(device, c, features(129, 512), weights(8, 512, 72), 2, prec, "ss+relu", cap=140)


@pytest.mark.parametrize("stride", [1, 2])
def test_cin512_bf16_stage(device, stride):
    """cnrma_sparse_conv_bf16 at Cin = 512, K = 27: fp32 accumulation of bf16 products against fp64 accumulation of the rounded
    operands, at the bar of tests/test_train_gpu.py"""
    c = block(320, lo=-4)
    run_conv(device, c, features(320, 512), weights(27, 512, 72), "stage", "bf16", stride=stride, epi="relu")


@pytest.mark.parametrize("rows,cin,cout", [(1, 96, 64), (65, 160, 72), (129, 96, 200), (300, 32, 65)])
def test_gather_once_bf16_edges(device, rows, cin, cout):
    """cnrma_sparse_conv_go_bf16 (the training forward; no epilogue, no live word) at the edge rows, slice counts and column
    tails, against fp64 accumulation of bf16-rounded operands"""
    from cnrma_amd import sparse as S
    c, f, W = block(rows, lo=-2), features(rows, cin), weights(27, cin, cout)
    _, exp = SO.conv(c, bf16_round(f), bf16_round(W), 3, 1, 1)
    Wd = torch.from_numpy(W).to(device)
    outs = []
    for _ in range(2):
        x = capacity_tensor(c, f, 1, device)
        with recorded_calls() as seen:
            outs.append(S._conv_go_bf16(x.F, (x.cs, x.cs, 3), S.weights_bf16_frag(Wd), cin, cout))
        assert [n for n in seen if n in CONV_ENTRIES] == ["cnrma_sparse_conv_go_bf16"]
    assert torch.equal(outs[0], outs[1])
    close(outs[0].cpu().numpy(), exp, bf16=True)


def run_convtr(device, c, f, W, ts, precision, epi="none", cap=None, value=POISON, seed=0):
    """S.conv_transpose_generative on (c, f), twice: entry, bit identity, exact child coordinates in the kernel's row order
    (child m = x << 2 | y << 1 | z of parent i at row 8 i + m), oracle values, live word = 8 x the parents', magnitude bound"""
    from cnrma_amd import sparse as S
    _, cin, cout = W.shape
    live, half = len(c), ts // 2
    cap_in = live if cap is None else cap
    _, of = SO.conv_transpose_generative(c, f, W, ts)
    kw, ref = epilogue(epi, seed, 0, 0, cout, device)
    m = np.arange(8)
    k_of_m = ((m >> 2) & 1) | (m & 2) | ((m & 1) << 2)
    exp = ref(of.reshape(8, live, cout)[k_of_m].transpose(1, 0, 2).reshape(8 * live, cout))
    off = np.stack((np.zeros(8, dtype=np.int64), (m >> 2) & 1, (m >> 1) & 1, m & 1), axis=1) * half
    exp_c = (c[:, None, :] + off[None]).reshape(8 * live, 4)
    entry = "cnrma_sparse_convtr_gen_" + (precision if cin % 32 == 0 else "f32")
    Wd = torch.from_numpy(W).to(device)
    outs = []
    for _ in range(2):
        x = capacity_tensor(c, f, ts, device, cap, value)
        with recorded_calls() as seen:
            y = S.conv_transpose_generative(x, Wd, precision=precision, **kw)
        assert [n for n in seen if n in CONV_ENTRIES] == [entry], seen
        outs.append(y)
    y = outs[0]
    assert y.cs.n == 8 * cap_in and y.cs.stride == half
    if cap is not None and cap > live:
        assert int(y.cs.n_dev[0]) == 8 * live
    assert (y.C[:8 * live].cpu().numpy().astype(np.int64) == exp_c).all()
    got = y.F[:8 * live]
    assert torch.equal(got, outs[1].F[:8 * live])
    close(got.cpu().numpy(), exp)
    if entry.endswith("f16x3"):
        assert float(y.amax.max()) == float(got.abs().max())
    return y, got


def _convtr_cases():
    cases = []
    wid = itertools.cycle([(32, 64), (96, 33), (160, 3), (32, 1), (96, 200)])
    for geo in ("rows1", "rows2", "rows63", "rows64", "rows65", "rows129", "twin", "neg", "lattice"):
        for prec in ("f16x3", "bf16x6", "f32"):
            cin, cout = next(wid)
            cases.append((prec, geo, cin, cout, 4 if geo == "neg" else 2, "none"))
    for epi in ("ss", "ss+relu", "ss+elu"):
        for prec in ("f16x3", "bf16x6", "f32"):
            cases.append((prec, "block", 96, 72, 2, epi))
    for cin in (1, 31, 33):
        cases.append(("f16x3", "rows65", cin, 33, 2, "ss+elu"))
    return cases


@pytest.mark.parametrize("case", _convtr_cases(), ids=lambda k: "-".join(map(str, k)))
def test_generative_transpose_edges(device, case):
    prec, geo, cin, cout, ts, epi = case
    c = GEOMETRY[geo](ts)
    run_convtr(device, c, features(len(c), cin), weights(8, cin, cout), ts, prec, epi)


def oracle_table(c_in, c_out, ks, ts):
    look = SO.Lookup(c_in)
    cols = []
    for off in SO.kernel_offsets(ks, ts):
        q = np.asarray(c_out, dtype=np.int64).copy()
        q[:, 1:] += off
        cols.append(look(q))
    return np.stack(cols, axis=1)


def test_children_table_of_two_scenes(device):
    """the 3x3x3 table of a generated child set (derived from the parents' table, no hash map) for two scenes with the same xyz:
    exact against the oracle's table, and the gather-once convolution on it against the oracle"""
    from cnrma_amd import sparse as S
    c = twin(block(40, 2, lo=-2))
    y, got = run_convtr(device, c, features(80, 32), weights(8, 32, 64), 2, "f16x3", "ss+relu")
    with recorded_calls() as seen:
        tab = y.cs.neighbours(y.cs, 3, 1).cpu().numpy()
    assert "cnrma_sparse_kernel_map_children" in seen
    cc = y.C.cpu().numpy().astype(np.int64)
    assert (tab == oracle_table(cc, cc, 3, 1)).all()
    W = weights(27, 64, 72)
    with settings(**FAMILY_SETTINGS["go"]), recorded_calls() as seen:
        z = S.conv(y, torch.from_numpy(W).to(device), 3, 1, precision="f16x3")          # on the derived table itself
    assert "cnrma_sparse_conv_go_f16x3" in seen
    close(z.F.cpu().numpy(), SO.conv(cc, got.cpu().numpy(), W, 3, 1, 1)[1])


# ---------------------------------------------------------------------------------------------------------------------
# item 7: the 16-bit fields of the coordinate key
# ---------------------------------------------------------------------------------------------------------------------
def _wrap_set(ts):
    """rows at both ends of the key range of a stride-`ts` level (the voxeliser admits |x| < 32767 at stride 1, so a stride-4
    level legally holds -32768 and 32764), on every axis, with real neighbours next to them"""
    lo, hi = -32768 if ts == 4 else -32766, 32766 // ts * ts
    pts = []
    for ax in range(3):
        for v in (lo, lo + ts, hi - ts, hi):
            p = [0, 0, 0]
            p[ax] = v
            pts.append([0] + p)
    pts += [[0, lo, lo, lo], [0, hi, hi, hi], [0, lo, hi, 0], [0, 0, 0, 0]]
    return np.unique(np.asarray(pts, dtype=np.int64), axis=0)


def test_no_neighbour_across_the_key_wrap(device):
    """coord_key() biases a coordinate by 32768 and keeps 16 bits: the probe 32764 + 4 of a stride-4 level wrapped to the key of
    the row at -32768 -- a false neighbour 65 536 voxels away (every builder, and the interpolation's far corner).  The
    builders now range-check their probes (hash_find_site): tables, pooled / strided maps, interpolation and a convolution
    through both families equal the oracle, whose keys are wide enough not to wrap."""
    from cnrma_amd import sparse as S
    c4 = _wrap_set(4)
    want = oracle_table(c4, c4, 3, 4)
    assert (want[np.nonzero(c4[:, 1] == 32764)[0]][:, 14] == -1).all()            # +x of the last column: nothing there
    for method in ("auto", "generic"):
        cs = capacity_tensor(c4, features(len(c4), 32), 4, device).cs
        assert (cs.neighbours(cs, 3, 4, method=method).cpu().numpy() == want).all(), method
    for fam in ("stage", "go"):
        run_conv(device, c4, features(len(c4), 32), weights(27, 32, 64), fam, "f16x3", ts=4, epi="relu")
    # the input-driven builder of the strided maps: stride 2 -> 4
    c2 = _wrap_set(2)
    out = SO.stride_coords(c2, 4)
    assert out[:, 1:].min() == -32768 and out[:, 1:].max() == 32764
    for ks in (3, 2, 1):
        cs = capacity_tensor(c2, features(len(c2), 32), 2, device).cs
        child = cs.strided(2)
        assert (child.C.cpu().numpy().astype(np.int64) == out).all()
        for method in ("auto", "generic"):
            cs._nbr.clear()
            assert (cs.neighbours(child, ks, 2, method=method).cpu().numpy() == oracle_table(c2, out, ks, 2)).all(), (ks, method)
    run_conv(device, c2, features(len(c2), 32), weights(27, 32, 33), "stage", "f32", stride=2, ts=2, epi="ss")
    # interpolation: a query one voxel above the last stride-4 site has its far corner at 32768
    q = np.asarray([[0, 32765, 1, 1], [0, 1, 32766, 2], [0, 3, 3, 32765], [0, -32767, -32766, -32765], [0, 32765, 32765, 32765]])
    score = features(len(c4), 1) + 3.0
    st = capacity_tensor(c4, score, 4, device)
    got = S.interpolate(st, torch.from_numpy(q.astype(np.int32)).to(device)).cpu().numpy()
    close(got, SO.interpolate(c4, score, 4, q))


# ---------------------------------------------------------------------------------------------------------------------
# B. capacity larger than the live count, dead rows poisoned
# ---------------------------------------------------------------------------------------------------------------------
CAPACITIES = {"plus1": (150, 151), "one_of_300": (1, 300), "tile_border": (128, 192)}


def _capacity_cases():
    cases = []
    for cname in CAPACITIES:
        for fam, prec in (("stage", "f32"), ("stage", "f16x3"), ("stage", "bf16x6"), ("stage", "bf16"), ("go", "f16x3"), ("go", "f32"),
                          ("pairs", "f16x3"), ("pairs", "f32")):
            cases.append((fam, prec, cname, POISON))
        for prec in ("f32", "f16x3", "bf16x6", "bf16"):
            cases.append(("stage2", prec, cname, POISON))
    cases += [("stage", "f16x3", "plus1", float("nan")), ("go", "f16x3", "tile_border", float("nan")),
              ("go", "f32", "plus1", float("nan")), ("pairs", "f16x3", "plus1", float("nan")),
              ("stage", "bf16x6", "tile_border", float("nan")),
              ("stage2", "f16x3", "tile_border", float("nan")), ("pairs", "f32", "one_of_300", float("nan"))]
    return cases


@pytest.mark.parametrize("case", _capacity_cases(), ids=lambda k: "-".join(map(str, k)))
def test_capacity_conv(device, case):
    """every convolution family on CoordSet(n=cap, n_dev=live) with poisoned dead rows (coordinates, features, residual): run_conv
    holds the live rows to the oracle on the live rows alone and the magnitude bound to their maximum; where the planner
    returns the same plan for cap and for live, the live rows equal the exact-size run bit for bit.  The stride-2 families (pair
    list, stage kernel under stride 2) also get an OUTPUT set of capacity `cap` with a live word (strided_with_capacity): their
    count / fill / epilogue kernels and out_amax reduction see no_cap > live, dead output rows and a poisoned residual"""
    fam, prec, cname, value = case
    live, cap = CAPACITIES[cname]
    stride = 2 if fam in ("pairs", "stage2") else 1
    c = lattice(live) if fam == "pairs" else block(live, lo=-3)
    cin, cout = (96, 68) if fam == "pairs" else (96, 72)
    f, W = features(live, cin), weights(27, cin, cout)
    got, amax, plan = run_conv(device, c, f, W, fam, prec, 3, stride, 1, "relu", cap, value, out_cap=cap if stride == 2 else None)
    ref, amax0, plan0 = run_conv(device, c, f, W, fam, prec, 3, stride, 1, "relu")
    same = lambda p: p if p is None else {k: v for k, v in p.items() if k != "workspace"}      # its bytes follow the capacity
    if same(plan) == same(plan0):
        assert torch.equal(got, ref) and amax == amax0
    else:
        assert cname != "plus1", (plan, plan0)                      # one dead row changes no launch choice at these sizes


@pytest.mark.parametrize("cname", list(CAPACITIES))
@pytest.mark.parametrize("prec,value", [("f16x3", POISON), ("bf16x6", POISON), ("f32", POISON), ("f16x3", float("nan"))])
def test_capacity_generative_transpose(device, prec, value, cname):
    live, cap = CAPACITIES[cname]
    c = block(live, 2, lo=-3)
    f, W = features(live, 96), weights(8, 96, 72)
    _, got = run_convtr(device, c, f, W, 2, prec, "ss+elu", cap, value)
    _, ref = run_convtr(device, c, f, W, 2, prec, "ss+elu")
    assert torch.equal(got, ref)


@pytest.mark.parametrize("cname", list(CAPACITIES))
@pytest.mark.parametrize("value", [POISON, float("nan")], ids=["3e38", "nan"])
def test_capacity_ops(device, cname, value):
    """max_pool, instance_norm, instance_norm_max_pool, union_add, prune, interpolate and SparseTensor.absmax.  First through
    their eager wrappers, which carry the live word of their INPUT (union_add, prune and the strided sets read their output
    count back: the derived sets are exact-size).  Then with a capacity on the OUTPUT side as well, the way a static trace
    runs them: max_pool / instance_norm_max_pool on strided_with_capacity(); union_add and prune through their C entries with
    out_cap / the kept count as a device word, a table and a convolution built on the resulting capacity-sized sets"""
    from cnrma_amd import sparse as S
    live, cap = CAPACITIES[cname]
    c = block(live, lo=-3)
    f = features(live, 32)
    x = lambda: capacity_tensor(c, f, 1, device, cap, value)
    # absmax: the live rows only
    assert float(x().absmax().max()) == float(np.abs(f).max())
    # max pooling: exact
    oc, of = SO.max_pool(c, f, 1)
    y = S.max_pool(x())
    assert y.cs.n == len(oc) and (y.C.cpu().numpy() == oc).all() and (y.F.cpu().numpy().astype(np.float64) == of).all()
    # instance norm: the statistics of the live rows only
    w, b = (1 + 0.1 * features(1, 32, 3)[0]), 0.1 * features(1, 32, 4)[0]
    wd, bd = torch.from_numpy(w).to(device), torch.from_numpy(b).to(device)
    exp = SO.instance_norm(f, w, b)
    y = S.instance_norm(x(), wd, bd, relu=True)
    close(y.F[:live].cpu().numpy(), SO.relu(exp))
    pc, pf = SO.max_pool(c, SO.relu(exp), 1)
    z = S.instance_norm_max_pool(x(), wd, bd)
    assert (z.C.cpu().numpy() == pc).all()
    close(z.F.cpu().numpy(), pf)
    assert float(z.amax.max()) == float(z.F.abs().max())
    assert torch.equal(z.F, S.max_pool(S.instance_norm(x(), wd, bd, relu=True)).F)
    # union_add with an overlapping set of its own capacity: counts and rows of the oracle, either operand order
    cb = block(live, lo=-1, seed=1)
    fb = features(live, 32, 5)
    b_ = capacity_tensor(cb, fb, 1, device, cap + 3 if cap > live else None, value)
    a_ = x()
    swap = b_.cs.n > a_.cs.n
    uc, uf = SO.union_add(cb, fb, c, f) if swap else SO.union_add(c, f, cb, fb)
    u = S.union_add(a_, b_)
    assert u.cs.n == len(uc) and (u.C.cpu().numpy() == uc).all()
    close(u.F.cpu().numpy(), uf)
    # prune: the kept live rows in order (the mask of a dead row is 0: sparse.topk_mask never keeps one)
    keep = np.zeros(cap, dtype=np.uint8)
    keep[:live] = np.random.RandomState(live).rand(live) < 0.6
    keep[0] = 1
    p_ = S.prune(x(), torch.from_numpy(keep).to(device), n_keep=int(keep.sum()))
    sel = np.nonzero(keep[:live])[0]
    assert (p_.C.cpu().numpy() == c[sel]).all() and (p_.F.cpu().numpy() == f[sel]).all()
    # ---- the same pooling operators with an OUTPUT set of capacity `cap` and a live word (strided_with_capacity: what a static
    # trace builds; the eager strided() above is exact-size): live output rows and the magnitude bound as before
    xs = x()
    child = strided_with_capacity(xs.cs, cap)
    n_o = len(oc)
    assert child.n == cap and int(child.n_dev[0]) == n_o and (child.C[:n_o].cpu().numpy() == oc).all()
    y = S.max_pool(xs)
    assert y.cs is child and y.F.shape[0] == cap and (y.F[:n_o].cpu().numpy().astype(np.float64) == of).all()
    xs = x()
    strided_with_capacity(xs.cs, cap)
    z2 = S.instance_norm_max_pool(xs, wd, bd)
    assert z2.F.shape[0] == cap and torch.equal(z2.F[:n_o], z.F)
    assert float(z2.amax.max()) == float(z.F.abs().max())
    # union_add as the static trace runs it, through its C entry (the eager wrapper reads n_out back and slices): the result is
    # a set of capacity out_cap with the live word n_out and the hash map the kernel extended; a convolution then runs on it
    ua, ub = (b_, a_) if swap else (a_, b_)
    na, nb = ua.cs.n, ub.cs.n
    m = S.CoordMap(na + nb, device)
    S.call("cnrma_sparse_build_map", S.ptr(ua.C), na, S.ptr(ua.cs.n_dev), S.ptr(m.keys), S.ptr(m.vals), m.cap, 0, S.stream())
    out_cap = na + nb - 2
    u_c = torch.from_numpy(poison_coords(uc[:1], na + nb).astype(np.int32)).to(device)
    u_f = torch.full((na + nb, 32), value, dtype=torch.float32, device=device)
    n_u = torch.empty(1, dtype=torch.int32, device=device)
    from cnrma_amd import _lib
    ws = torch.empty(_lib.load().cnrma_union_workspace_bytes(nb), dtype=torch.uint8, device=device)
    S.call("cnrma_sparse_union_add_f32", S.ptr(ua.C), S.ptr(ua.F), na, S.ptr(ua.cs.n_dev), S.ptr(ub.C), S.ptr(ub.F), nb,
           S.ptr(ub.cs.n_dev), 32, S.ptr(m.keys), S.ptr(m.vals), m.cap, S.ptr(u_c), S.ptr(u_f), out_cap, S.ptr(n_u), S.ptr(ws), S.stream())
    assert int(n_u[0]) == len(uc) and (u_c[:len(uc)].cpu().numpy() == uc).all() and torch.equal(u_f[:len(uc)], u.F)
    ucs = S.CoordSet(u_c, 1, m, n=out_cap, n_dev=n_u)
    Wu = weights(27, 32, 64)
    with settings(**FAMILY_SETTINGS["stage"]):
        v = S.conv(S.SparseTensor(u_f[:out_cap], ucs), torch.from_numpy(Wu).to(device), 3, 1, precision="f16x3")
    close(v.F[:len(uc)].cpu().numpy(), SO.conv(uc, u.F.cpu().numpy(), Wu, 3, 1, 1)[1])
    assert float(v.amax.max()) == float(v.F[:len(uc)].abs().max())
    # prune as the static trace runs it: the keep-mask from topk_mask with the live word (dead scores are poison 3e38, the
    # largest of all: only the live mask keeps them out), k above the live count, the kept count n_sel as the output's live word
    from cnrma_amd.rma import mask_to_index
    scores = np.random.RandomState(live + 1).rand(live).astype(np.float32)
    xs = x()
    for k in (max(1, live // 2), live + 1):
        mask = S.topk_mask(poison_rows(scores[:, None], cap, device, POISON).view(-1), k, xs.cs.n_dev)
        kept = np.sort(np.argsort(-scores, kind="stable")[:k])
        assert (mask.cpu().numpy() == np.isin(np.arange(cap), kept)).all()
        sel, n_sel = mask_to_index(mask)
        p_c = torch.from_numpy(poison_coords(c[:1], k).astype(np.int32)).to(device)
        p_f = torch.full((k, 32), value, dtype=torch.float32, device=device)
        S.call("cnrma_sparse_prune_f32", S.ptr(xs.C), S.ptr(xs.F), cap, S.ptr(xs.cs.n_dev), 32, S.ptr(sel), S.ptr(p_c), S.ptr(p_f), S.stream())
        assert int(n_sel[0]) == len(kept) and (p_c[:len(kept)].cpu().numpy() == c[kept]).all()
        assert (p_f[:len(kept)].cpu().numpy() == f[kept]).all()
        pcs = S.CoordSet(p_c, 1, None, n=k, n_dev=n_sel)
        tab = pcs.neighbours(pcs, 3, 1)[:len(kept)].cpu().numpy()
        assert (tab == oracle_table(c[kept], c[kept], 3, 1)).all()
    # interpolation: a poisoned score set, poisoned queries
    score = features(live, 1, 6)
    q = block(2 * live, lo=-4, seed=2)
    qd = torch.from_numpy(poison_coords(q, 2 * live + 9).astype(np.int32)).to(device)
    nq = torch.tensor([2 * live], dtype=torch.int32, device=device)
    got = S.interpolate(capacity_tensor(c, score, 1, device, cap, value), qd, nq)
    close(got[:2 * live].cpu().numpy(), SO.interpolate(c, score, 1, q))


@pytest.mark.parametrize("cname", list(CAPACITIES))
def test_capacity_tables(device, cname):
    """the neighbour tables (symmetric, strided k3 / k2 / k1, generic, generated children), the strided set and the tile unions
    of a poisoned set: the live rows' entries equal the oracle's and never name a row >= live"""
    from cnrma_amd import sparse as S
    live, cap = CAPACITIES[cname]
    c = block(live, 2, lo=-3)
    cs = lambda: capacity_tensor(c, features(live, 32), 2, device, cap).cs
    want = oracle_table(c, c, 3, 2)
    for method in ("auto", "generic"):
        s_ = cs()
        with recorded_calls() as seen:
            tab = s_.neighbours(s_, 3, 2, method=method)[:live].cpu().numpy()
        assert ("cnrma_sparse_kernel_map_symmetric" if method == "auto" else "cnrma_sparse_kernel_map") in seen
        assert (tab == want).all() and tab.max() < live
    out = SO.stride_coords(c, 4)
    for ks in (3, 2, 1):
        for method in ("auto", "generic"):
            s_ = cs()
            child = s_.strided(2)
            assert child.n == len(out) and (child.C.cpu().numpy() == out).all()
            with recorded_calls() as seen:
                tab = s_.neighbours(child, ks, 2, method=method).cpu().numpy()
            assert ("cnrma_sparse_kernel_map_strided" if method == "auto" else "cnrma_sparse_kernel_map") in seen
            assert (tab == oracle_table(c, out, ks, 2)).all() and tab.max() < live
    # the strided set and its tables with a CAPACITY on the output side too (hash and, on a Morton-sorted set, sort builder)
    for ks in (3, 2, 1):
        for method in ("auto", "generic"):
            s_ = cs()
            child = strided_with_capacity(s_, cap)
            n_o = len(out)
            assert int(child.n_dev[0]) == n_o and (child.C[:n_o].cpu().numpy() == out).all()
            tab = s_.neighbours(child, ks, 2, method=method)[:n_o].cpu().numpy()
            assert tab.shape[0] == n_o and (tab == oracle_table(c, out, ks, 2)).all() and tab.max() < live
    pts = block(live, lo=-3)[:, 1:].astype(np.float32) + 0.5
    cm = S.voxelize(torch.from_numpy(pts).to(device), torch.from_numpy(features(live, 4)).to(device), 1.0)[0].C.cpu().numpy().astype(np.int64)
    exact = capacity_tensor(cm, features(live, 4), 1, device).cs
    exact.sorted = True
    with recorded_calls() as seen:
        want_c = exact.strided(2).C.cpu().numpy()
    assert "cnrma_sparse_stride_coords_sorted" in seen
    assert sorted(map(tuple, want_c)) == sorted(map(tuple, SO.stride_coords(cm, 2)))
    s_ = capacity_tensor(cm, features(live, 4), 1, device, cap).cs
    s_.sorted = True
    child = strided_with_capacity(s_, cap, by_sort=True)
    assert int(child.n_dev[0]) == len(want_c) and (child.C[:len(want_c)].cpu().numpy() == want_c).all()
    tab = s_.neighbours(child, 3, 1)[:len(want_c)].cpu().numpy()
    assert (tab == oracle_table(cm, want_c, 3, 1)).all() and tab.max() < live
    # generated children of a poisoned parent set
    y, _ = run_convtr(device, c, features(live, 32), weights(8, 32, 64), 2, "f32", cap=cap)
    with recorded_calls() as seen:
        tab = y.cs.neighbours(y.cs, 3, 1)[:8 * live].cpu().numpy()
    assert "cnrma_sparse_kernel_map_children" in seen
    cc = y.C[:8 * live].cpu().numpy().astype(np.int64)
    assert (tab == oracle_table(cc, cc, 3, 1)).all() and tab.max() < 8 * live
    # tile unions of the live tiles: every listed row is live, every (row, offset) resolves to the table's entry
    s_ = cs()
    tu = S.tile_union(s_, s_, 3, 2).cpu()
    n_t, live_t = (cap + 63) // 64, (live + 63) // 64
    al = lambda b: (b + 255) // 256 * 256
    hdr = tu[:n_t * 84 * 4].view(torch.int32).view(n_t, 84).numpy()
    rows = tu[al(n_t * 84 * 4):al(n_t * 84 * 4) + n_t * 1728 * 4].view(torch.int32).view(n_t, 1728).numpy()
    o2 = al(n_t * 84 * 4) + al(n_t * 1728 * 4)
    lidx = tu[o2:o2 + n_t * 1728 * 2].view(torch.int16).view(n_t, 64, 27).numpy().astype(np.int64) & 0xFFFF
    for t in range(live_t):
        done = 0
        for g in range(hdr[t, 0]):
            mask, ub, un = int(hdr[t, 1 + 3 * g]) & 0xFFFFFFFF, hdr[t, 2 + 3 * g], hdr[t, 3 + 3 * g]
            u = rows[t, ub:ub + un]
            assert 0 < un <= S.GO_UMAX and (mask & done) == 0 and u.min() >= 0 and u.max() < live
            done |= mask
            for k in range(27):
                if (mask >> k) & 1:
                    for r in range(min(64, live - 64 * t)):
                        w = want[64 * t + r, k]
                        assert (lidx[t, r, k] == S.GO_UMAX) if w < 0 else (u[lidx[t, r, k]] == w)
        assert all(((done >> k) & 1) == int((want[64 * t:64 * t + 64, k] >= 0).any()) for k in range(27))


def test_live_zero(device):
    """an empty scene under a capacity: no error, empty derived sets, a zero magnitude bound"""
    from cnrma_amd import sparse as S
    c = np.zeros((0, 4), dtype=np.int64)
    x = capacity_tensor(c, np.zeros((0, 64), dtype=np.float32), 1, device, 70)
    assert float(x.absmax().max()) == 0.0
    W = torch.from_numpy(weights(27, 64, 72)).to(device)
    res = poison_rows(np.zeros((0, 72), dtype=np.float32), 70, device)
    for fam in ("stage", "go"):
        for prec in ("f16x3", "f32"):
            with settings(**FAMILY_SETTINGS[fam]):
                y = S.conv(x, W, 3, 1, residual=res, act="relu", precision=prec)
            assert y.cs.n == 70 and int(y.cs.n_dev[0]) == 0
            if prec == "f16x3":
                assert float(y.amax.max()) == 0.0
    assert S.conv(x, W, 3, 2).cs.n == 0 and S.max_pool(x).cs.n == 0
    up = S.conv_transpose_generative(capacity_tensor(c, np.zeros((0, 64), dtype=np.float32), 2, device, 70),
                                     torch.from_numpy(weights(8, 64, 32)).to(device))
    assert up.cs.n == 560 and int(up.cs.n_dev[0]) == 0 and float(up.amax.max()) == 0.0
    u = S.union_add(x, capacity_tensor(block(5), features(5, 64), 1, device, 9))
    assert u.cs.n == 5 and (u.C.cpu().numpy() == block(5)).all() and (u.F.cpu().numpy() == features(5, 64)).all()
    # instance norm (its statistics divide by the live count: the outputs of an empty scene are undefined, the call is not an
    # error), the fused norm + pooling (empty output, zero bound), prune, interpolation of live queries on an empty score set,
    # and the table builders / tile unions (nothing to write; the calls must go through)
    wd = torch.ones(64, device=device)
    assert S.instance_norm(x, wd, wd, relu=True).F.shape == (70, 64)
    z = S.instance_norm_max_pool(x, wd, wd)
    assert z.cs.n == 0 and float(z.amax.max()) == 0.0
    p_ = S.prune(x, torch.zeros(70, dtype=torch.uint8, device=device))
    assert p_.cs.n == 0
    q = torch.from_numpy(block(9).astype(np.int32)).to(device)
    empty_score = capacity_tensor(c, np.zeros((0, 1), dtype=np.float32), 1, device, 70)
    assert (S.interpolate(empty_score, q).cpu().numpy() == 0).all()
    full = capacity_tensor(block(9), features(9, 1), 1, device)
    S.interpolate(full, x.C, x.cs.n_dev)                                       # no live query: nothing written, no error
    for method in ("auto", "generic"):
        e = capacity_tensor(c, np.zeros((0, 64), dtype=np.float32), 1, device, 70).cs
        e.neighbours(e, 3, 1, method=method)
        S.tile_union(e, e, 3, 1)
        child = strided_with_capacity(e, 70)
        assert int(child.n_dev[0]) == 0
        e.neighbours(child, 3, 1, method=method)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------
# C. every choice of the product launchers
# ---------------------------------------------------------------------------------------------------------------------
# capacities on both sides of every threshold of plan_conv / go2_plan / the workspace queries: rows 1 000 / 4 000 / 16 384 /
# 40 000 / 65 536 (no split workspace from there) / 200 000; 32 and 2 048 tiles of 64 rows; 384 blocks at 1, 2 and 4 column tiles
# of 64-row tiles and at 128-row tiles
GRID_CAPS = (1, 64, 65, 300, 999, 1000, 1984, 1985, 2500, 3999, 4000, 6080, 6081, 12000, 12224, 12225, 16383, 16384, 24512, 24513,
             30000, 39999, 40000, 49024, 49025, 50000, 65535, 65536, 131008, 131009, 140000, 199999, 200000, 250000)
GRID_CIN = (16, 32, 64, 96, 160, 256, 512)
GRID_COUT = (1, 32, 33, 64, 65, 96, 127, 128, 160, 200, 255, 256, 512)
GRID_GO_COUT = (64, 65, 96, 127, 128, 160, 200, 256, 512)

# (precision, capacity, Cin, Cout, K,   tile shape, split over the offsets) -- the last two are the plan conv_plan must return
STAGE_CASES = [
    ("bf16", 16384, 32, 128, 1, "128x128", False),
    ("bf16", 16384, 32, 128, 27, "128x128", True),
    ("bf16", 300, 32, 32, 1, "128x32", False),
    ("bf16", 300, 32, 32, 27, "128x32", True),
    ("bf16", 200000, 64, 33, 1, "128x64", False),
    ("bf16", 300, 32, 256, 1, "64x128", False),
    ("bf16", 300, 32, 256, 27, "64x128", True),
    ("bf16", 300, 32, 33, 1, "64x64", False),
    ("bf16", 300, 32, 33, 27, "64x64", True),
    ("bf16x6", 16384, 32, 128, 1, "128x128", False),
    ("bf16x6", 16384, 32, 128, 27, "128x128", True),
    ("bf16x6", 300, 32, 32, 1, "128x32", False),
    ("bf16x6", 300, 32, 32, 27, "128x32", True),
    ("bf16x6", 4000, 32, 33, 1, "128x64", False),
    ("bf16x6", 4000, 32, 33, 27, "128x64", True),
    ("bf16x6", 300, 32, 256, 1, "64x128", False),
    ("bf16x6", 300, 32, 256, 27, "64x128", True),
    ("bf16x6", 300, 32, 33, 1, "64x64", False),
    ("bf16x6", 300, 32, 33, 27, "64x64", True),
    ("f16x3", 16384, 32, 128, 1, "128x128", False),
    ("f16x3", 16384, 32, 128, 27, "128x128", True),
    ("f16x3", 300, 32, 32, 1, "128x32", False),
    ("f16x3", 300, 32, 32, 27, "128x32", True),
    ("f16x3", 200000, 64, 33, 1, "128x64", False),
    ("f16x3", 300, 32, 256, 1, "64x128", False),
    ("f16x3", 300, 32, 256, 27, "64x128", True),
    ("f16x3", 300, 32, 33, 1, "64x64", False),
    ("f16x3", 300, 32, 33, 27, "64x64", True),
    ("f32", 16384, 32, 128, 1, "128x128", False),
    ("f32", 16384, 16, 128, 27, "128x128", True),
    ("f32", 300, 32, 32, 1, "128x32", False),
    ("f32", 300, 32, 32, 27, "128x32", True),
    ("f32", 16384, 32, 33, 1, "128x64", False),
    ("f32", 16384, 32, 33, 27, "128x64", True),
    ("f32", 300, 32, 33, 1, "64x64", False),
    ("f32", 300, 32, 33, 27, "64x64", True),
    # the large-capacity tiles once more at their real widths, and the 128x64 tile of f16x3 / bf16 with 27 offsets
    ("f16x3", 250000, 64, 64, 27, "128x64", False),
    ("bf16", 250000, 64, 64, 27, "128x64", False),
    ("f16x3", 20000, 128, 128, 27, "128x128", True),
    ("bf16x6", 140000, 64, 128, 27, "128x128", False),
    ("f32", 50000, 32, 64, 27, "128x64", False),
    ("bf16x6", 50000, 64, 64, 27, "128x64", False),
]
# (capacity, Cin, Cout, residual,   tile columns, "whole" / "split" / "uneven" (last split shorter), work order) -- the plan
# conv_go_plan must return; the residual is added in the kernel by a whole launch and in the reduction by a split one
GO_CASES = [
    (131009, 32, 64, 0, 64, "whole", "plain"),
    (131009, 32, 64, 1, 64, "whole", "plain"),
    (300, 32, 64, 0, 64, "whole", "tiles->xcd"),
    (300, 32, 64, 1, 64, "whole", "tiles->xcd"),
    (300, 160, 65, 1, 64, "split", "groups->xcd"),
    (300, 64, 64, 1, 64, "split", "tiles->xcd"),
    (12225, 160, 64, 1, 64, "uneven", "tiles->xcd"),
    (131009, 32, 128, 0, 128, "whole", "plain"),
    (131009, 32, 128, 1, 128, "whole", "plain"),
    (300, 32, 128, 0, 128, "whole", "tiles->xcd"),
    (300, 32, 128, 1, 128, "whole", "tiles->xcd"),
    (300, 160, 160, 1, 128, "split", "groups->xcd"),
    (300, 64, 128, 1, 128, "split", "tiles->xcd"),
    (1984, 512, 512, 1, 128, "uneven", "groups->xcd"),
    (12225, 160, 128, 1, 128, "uneven", "tiles->xcd"),
    # the benchmark's own classes: 140 000 and 250 000 rows in plain order, 20 000 and 50 000 between
    (250000, 64, 64, 1, 64, "whole", "plain"),
    (140000, 64, 128, 1, 128, "whole", "plain"),
    (20000, 256, 256, 1, 128, "whole", "tiles->xcd"),
    (50000, 128, 128, 1, 128, "whole", "tiles->xcd"),
]


def _live_rows(cap):
    return cap - 37 if cap <= 400 else 333


def test_every_product_launcher_choice_has_a_case():
    """the planners over a grid of (capacity, Cin, Cout, K, slices / residual) that crosses each of their thresholds: every distinct
    (precision, shape, split, prefetch) of conv_plan and (columns, split, uneven last split, order, residual in the kernel) of
    conv_go_plan must be the plan of one of the cases test_stage_launcher_choice / test_gather_once_launcher_choice run against
    the oracle -- a new threshold or variant without a case fails here"""
    from cnrma_amd import _lib
    assert not _lib.experiments_active() and not hasattr(_lib.load(), "cnrma_debug_conv_tuning")
    want = set()
    for prec in ("f32", "f16x3", "bf16x6", "bf16"):
        for cap, cin, cout, (K, slices) in itertools.product(GRID_CAPS, GRID_CIN, GRID_COUT, ((1, 1), (8, 1), (27, 1), (1, 8))):
            want.add(stage_key(prec, cap, cin, cout, K, slices))
    have = {stage_key(*case[:5]) for case in STAGE_CASES}
    assert want - have == set(), sorted(want - have)
    want = {go_key(cap, cin, cout, r) for cap, cin, cout, r in itertools.product(GRID_CAPS, GRID_CIN[1:], GRID_GO_COUT, (0, 1))}
    have = {go_key(*case[:4]) for case in GO_CASES}
    assert want - have == set(), sorted(want - have)
    assert len(want) >= 15 and {k[3] for k in want} == {"plain", "groups->xcd", "tiles->xcd"}


@pytest.mark.parametrize("case", STAGE_CASES, ids=lambda k: "-".join(map(str, k)))
def test_stage_launcher_choice(device, case):
    """one stage-kernel plan of the product launcher (reached through the capacity) with scale + shift + residual + activation,
    against the oracle.  The plan written in the case is what conv_plan must return for these sizes; that the launch follows it
    cannot be observed from outside -- it rests on launch_conv and cnrma_sparse_conv_plan calling the same pure plan_conv()"""
    prec, cap, cin, cout, K, shape, split = case
    live = _live_rows(cap)
    c = block(live, lo=-4)
    epi = "relu" if (cap + cout + K) % 2 else "elu"
    _, _, plan = run_conv(device, c, features(live, cin), weights(K, cin, cout), "stage", prec, 3 if K == 27 else 1, 1, 1, epi, cap)
    assert (plan["shape"], plan["splits"] > 1, plan["prefetch"]) == (shape, split, 1)


@pytest.mark.parametrize("case", GO_CASES, ids=lambda k: "-".join(map(str, k)))
@pytest.mark.parametrize("prec", ["f16x3", "f32"])
def test_gather_once_launcher_choice(device, prec, case):
    """one gather-once plan of the product launcher with the full epilogue (residual 0: scale + shift only); split plans add
    their slabs and apply all four epilogue terms in the reduction.  The plan written in the case is what conv_go_plan must
    return; the launchers call the same pure go2_plan()"""
    cap, cin, cout, residual, columns, kind, order = case
    live = _live_rows(cap)
    c = block(live, lo=-4)
    epi = ("relu" if (cap + cout) % 2 else "elu") if residual else "ss"
    _, _, plan = run_conv(device, c, features(live, cin), weights(27, cin, cout), "go", prec, epi=epi, cap=cap)
    uneven = plan["splits"] > 1 and (cin // 32) % plan["slices_per_split"] != 0
    assert (plan["columns"], ("uneven" if uneven else "split") if plan["splits"] > 1 else "whole", plan["order"]) == (columns, kind, order)
    assert plan["residual_in_kernel"] == (bool(residual) and kind == "whole")
