"""GPU tests (-m gpu) of the TRAINING half of the sparse engine at edge shapes, widths and live counts, kernel by kernel
against a numpy fp64 reference of a few lines (oracle/sparse_oracle.py: conv_backward, batch_norm_train[_backward],
max_pool_backward; the new ones are pinned by central differences in tests/test_sparse_oracle_cpu.py), through
cnrma_amd.sparse and the PRODUCT library only (conv_tuning() is never called).

tests/test_train_gpu.py and tests/test_sparse_gpu.py drive what train_step differentiates through with a few thousand random
rows, widths that are multiples of 32 and capacities equal to the row count.  The forward half got its edge suite in
tests/test_sparse_edges_gpu.py; this is the same for the backward kernels:

  A  conv_wgrad_block_kernel<BF16, V2> through cnrma_sparse_conv_wgrad_f32 / _bf16 called directly on synthetic neighbour
     tables (an all -1 column, an all -1 row, nbr == NULL with K = 1): slabs prefilled with NaN (every element must be
     written), every chunk's slab against fp64 on its own rows, chunks behind the live rows exactly zero, twice bit-identical.
  B  kernel_map_transpose_kernel alone against numpy.
  C  the data gradient (and, from the same backward, the weight gradient) through conv_autograd on the degenerate coordinate
     sets of the forward suite, mirrored and transposed-table form asserted by the entries that ran.
  D  conv_wgrad_go_kernel called directly on tile_union(...) and through autograd with WGRAD_GO = True.
  E  the BatchNorm training kernels against fp64, their bar measured from torch's own fp32 kernels on the same inputs.
  F  _MaxPoolFn.backward by value and the fused _ConvBnActFn node against the fp64 composition and its unfused form.

Where the items of the issue live:
  1 block kernel, XCD-first decode (by_chunk) .. test_wgrad_block[*-bychunk], test_wgrad_block_chunk_counts[32|33|39]
  2 chunk count no multiple of 8 ............... test_wgrad_block_chunk_counts[31|33|39], test_wgrad_block[*-bychunk] (33 chunks)
  3 last 32-row step short of 32 rows .......... test_wgrad_block[rows1|31|33|255|257-*]
  4 even rows_per_chunk off the 32-multiple .... test_wgrad_block[*-rpc34*], test_wgrad_block_two_rows_per_chunk
  5 the scalar V2 = false path ................. test_wgrad_block[*-1x1|3x5|65x64-*], test_wgrad_block_identity_table
  6 channel tails in the 2nd / 3rd tile ........ test_wgrad_block[*-65x64|66x130|130x62-*]
  7 the no_dev live count of the wgrad entries . test_wgrad_block[*-bychunk], test_wgrad_block_live_counts, test_wgrad_go_capacity
  8 gather-once: a part with no tiles .......... test_wgrad_go_direct (parts 16 / 17 / > live tiles), test_wgrad_go_capacity
  9 gather-once: the by_part decode ............ test_wgrad_go_direct / _capacity / _partial_tile_with_several_groups (parts 16, 17)
 10 gather-once: partial tile, several groups .. test_wgrad_go_partial_tile_with_several_groups
 11 gather-once: odd union counts .............. test_wgrad_go_direct[rows1-*|rows63-*] (asserted on the CPU from the table)
 12 gather-once: fewer than 256 rows ........... test_wgrad_go_direct, test_wgrad_go_through_autograd
 13 gather-once: live < capacity ............... test_wgrad_go_capacity
 14 cnrma_bn_backward_f32 (never called) ....... test_bn_backward_any_width
 15 bn train: 256 % C != 0 ..................... test_bn_train[*-c36|c100|c252-*]
 16 bn train: ELU with a residual .............. test_bn_train[*-elu-res]
 17 bn train: n = 2, constant / offset column .. test_bn_train[n2-*] (unbiased factor 2), every case with n > 3 (columns 1, 2)
 18 bn train: against fp64 ..................... test_bn_train, test_bn_train_grid_stride
 19 _MaxPoolFn.backward by value ............... test_max_pool_gradient, test_relu_max_pool_gradient
 20 the fused _ConvBnActFn node ................ test_fused_conv_bn_act, test_fused_conv_bn_act_fallbacks
 21 kernel_map_transpose_kernel ................ test_kernel_map_transpose, test_data_gradient[*-transposed]
 22 data gradient, mirrored / transposed ....... test_data_gradient, test_data_gradient_on_the_gather_once_kernel
 23 refused arguments (return before a launch) . test_refused_arguments
  (no kernel fault was met and no value check failed on the MI355X: nothing in csrc/sparse.hip or sparse.py had to change.
   What the file can see was checked on scratch builds with one memory-safe defect each -- an offset / tile decode that is no
   bijection in either branch of the block kernel, the live count ignored by the block kernel or by the transpose, the by_part
   decode, an empty part that skips its store, stale local indices in the in-place staging path, the wrong statistic as the
   mean in bn_backward_apply_kernel, a column-sum stride that is wrong only where 256 % C != 0, an apply kernel without its
   grid-stride turn, a pooling gradient to every child, an unmirrored mirrored form: each fails tests of the item it belongs
   to.  One does not: writing row 0 instead of zeros into the image row behind an odd union count (`u + 1 < cnt` in the
   producers' store_rows) changes no result, because no local index names that row.)

Bars: fp32 weight and data gradients max|got - ref| < 2e-6 max|ref| against fp64 (test_conv_backward_vs_oracle); bf16 entries
2e-5 max|ref| against fp64 on bf16-rounded operands (tests/test_train_gpu.py); empty slabs, live-versus-exact-size runs, repeat
runs and every index output exact, bit for bit.  BatchNorm: for every output and column class the error of torch's own fp32
nn.BatchNorm1d (+ add + activation) against the same fp64 reference is measured on the GPU; the kernel's bar is 4 x that
error with a floor of 1e-6 max|ref| (the kernels keep fp64 sums: they should not be worse than torch; the margin covers
another rounding order), and on ordinary columns the tolerances of test_batch_norm_train_kernels_match_torch stay as an
upper bound.  The ReLU kink is kept out of every comparison by construction (helpers.clear_of_kink), never by a mask."""
import itertools

import numpy as np
import pytest
import torch

from helpers import POISON, capacity_tensor, clear_of_kink, poison_rows
from oracle import sparse_oracle as SO
from test_sparse_edges_gpu import CONV_ENTRIES, GEOMETRY, bf16_round, block, features, recorded_calls, settings, weights

pytestmark = pytest.mark.gpu
F32_BAR, BF16_BAR = 2e-6, 2e-5
EPS = 1e-5


# ---------------------------------------------------------------------------------------------------------------------
# plumbing
# ---------------------------------------------------------------------------------------------------------------------
def product_library():
    from cnrma_amd import _lib
    assert not _lib.experiments_active()
    return _lib.load()


def dev(a, device, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(device)


def scrub(device, *shapes):
    """cnrma_amd.sparse allocates its own outputs with torch.empty, so a test cannot prefill them; instead the free memory
    they will most likely come from is filled with NaN: torch's cache is released and three NaN tensors of every shape are
    parked in it.  An element that a kernel leaves unwritten then reads NaN -- not the equal value that another run (the
    torch reference, the same case a moment ago) left in a recycled block, which is how an apply kernel without its
    grid-stride turn once passed a case here"""
    torch.cuda.synchronize(device)
    torch.cuda.empty_cache()
    junk = [torch.full(tuple(sh), float("nan"), dtype=torch.float32, device=device) for sh in shapes for _ in range(3)]
    del junk


def assert_close(got, ref, bar, what=""):
    """the issue's bar: max|got - ref| < bar * max|ref|; a reference that is all zero must be met exactly"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape and np.isfinite(got).all(), what
    scale = float(np.abs(ref).max()) if ref.size else 0.0
    if scale == 0.0:
        assert not got.any(), what
        return
    err = float(np.abs(got - ref).max())
    assert err < bar * scale, (what, err, bar * scale)


def same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32))


def wgrad_ref(F, nbr, G, r0=0, r1=None):
    """gW[k] = sum over the output rows r0 <= o < r1 of F[nbr[o, k]]^T G[o] in fp64 (nbr None: the identity table, K = 1)"""
    F, G = np.asarray(F, dtype=np.float64), np.asarray(G, dtype=np.float64)
    r1 = len(G) if r1 is None else r1
    K = 1 if nbr is None else nbr.shape[1]
    out = np.zeros((K, F.shape[1], G.shape[1]))
    for k in range(K):
        idx = np.arange(r0, r1) if nbr is None else nbr[r0:r1, k]
        m = idx >= 0
        if m.any():
            out[k] = F[idx[m]].T @ G[r0:r1][m]
    return out


def synthetic_table(n_out, K, n_in, seed):
    """nbr [n_out, K] with entries in [-1, n_in): a third of them -1, one all -1 column (K > 1), one all -1 row (n_out > 1)"""
    rng = np.random.RandomState(seed)
    nbr = rng.randint(0, n_in, size=(n_out, K)).astype(np.int32)
    nbr[rng.rand(n_out, K) < 0.3] = -1
    if K > 1:
        nbr[:, K // 2] = -1
    if n_out > 1:
        nbr[n_out // 2] = -1
    return nbr


def operands(n_in, n_out, cin, cout, seed):
    """features and gradient rows with a mean (0.75): no weight-gradient element is a sum that cancels to nothing, so the bar
    relative to max|ref| means the same at a 1 x 1 slab as at a 64 x 64 one"""
    rng = np.random.RandomState(seed)
    return (rng.randn(n_in, cin) + 0.75).astype(np.float32), (rng.randn(n_out, cout) + 0.75).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------------
# A. weight gradient, block kernel
# ---------------------------------------------------------------------------------------------------------------------
DEAD_ROWS = 4       # poisoned rows behind the input features: what a dead table row points at (allocated, visible in any sum)


def run_wgrad_block(device, F, nbr, G, rpc, bf16, cap=None, poison=POISON):
    """cnrma_sparse_conv_wgrad_f32 / _bf16 on the live rows (F [n_in], nbr [live, K] or None, G [live]) with a capacity of
    `cap` output rows: behind the live count the gradient rows are poison and the table rows point at poisoned feature rows.
    NaN-prefilled slabs, run twice -> slabs [chunks, K, Cin, Cout] (bit-identical, every element written)"""
    from cnrma_amd import sparse as S
    lib = product_library()
    live, cout = G.shape
    n_in, cin = F.shape
    K = 1 if nbr is None else nbr.shape[1]
    cap = live if cap is None else cap
    no_dev = None
    if cap > live:
        no_dev = torch.tensor([live], dtype=torch.int32, device=device)
        Gd = poison_rows(G, cap, device, poison)
        Fd = poison_rows(F, (cap if nbr is None else n_in + DEAD_ROWS), device, poison)
        if nbr is not None:
            dead = np.random.RandomState(live).randint(0, n_in + DEAD_ROWS, size=(cap - live, K))
            nbr = np.concatenate((nbr, dead.astype(np.int32)))
    else:
        Gd, Fd = dev(G, device), dev(F, device)
    nd = None if nbr is None else dev(nbr, device, np.int32)
    assert nd is None or (int(nd.max()) < Fd.shape[0] and int(nd.min()) >= -1 and nd.shape == (cap, K))
    assert Gd.shape == (cap, cout) and (nbr is not None or Fd.shape[0] == cap)
    chunks = lib.cnrma_sparse_conv_wgrad_chunks(cap, rpc)
    assert chunks == -(-cap // rpc)
    outs = []
    for _ in range(2):
        slabs = torch.full((chunks, K, cin, cout), float("nan"), dtype=torch.float32, device=device)
        S.call("cnrma_sparse_conv_wgrad_bf16" if bf16 else "cnrma_sparse_conv_wgrad_f32", S.ptr(Fd), cin, S.ptr(nd), K, S.ptr(Gd),
               cout, cap, S.ptr(no_dev), rpc, S.ptr(slabs), S.stream())
        outs.append(slabs.cpu().numpy())
    assert not np.isnan(outs[0]).any(), "an element of a slab was not written"
    assert same_bits(outs[0], outs[1]), "run to run"
    return outs[0]


def check_wgrad_block(slabs, F, nbr, G, rpc, bf16):
    """every chunk's slab against fp64 on the chunk's live rows (bf16: on rounded operands), chunks behind the live rows and
    the slabs of an all -1 column exactly zero, and the sum of the slabs against the whole gradient"""
    Fo, Go = (bf16_round(F), bf16_round(G)) if bf16 else (F, G)
    bar = BF16_BAR if bf16 else F32_BAR
    live = len(G)
    for ch in range(slabs.shape[0]):
        r0, r1 = ch * rpc, min(live, (ch + 1) * rpc)
        if r0 >= live:
            assert not slabs[ch].any(), "chunk %d lies behind the live rows" % ch
        else:
            assert_close(slabs[ch], wgrad_ref(Fo, nbr, Go, r0, r1), bar, "chunk %d" % ch)
    if nbr is not None and nbr.shape[1] > 1:
        assert not slabs[:, nbr.shape[1] // 2].any(), "the offset without a neighbour"
    if live:
        assert_close(slabs.astype(np.float64).sum(0), wgrad_ref(Fo, nbr, Go), bar, "sum of the slabs")


ROWS = (1, 31, 32, 33, 255, 256, 257)
WIDTHS = ((1, 1), (3, 5), (2, 2), (64, 64), (65, 64), (66, 130), (130, 62))
OFFSETS = (1, 8, 27)
RPC = (32, 34, 256)


def _block_cases():
    """(precision, live rows, capacity or None, rows_per_chunk, K, Cin, Cout), listed, not crossed: in each precision and on
    either side of by_chunk (32 chunks) every row count once, with every width, offset count and rows_per_chunk.  Below 32
    chunks the capacity is the row count (no live word); from 32 chunks on the row counts are LIVE counts under a capacity of
    32 * rows_per_chunk + 2 rows = 33 chunks (no multiple of 8: five blocks of the last XCD round return early)."""
    cases = []
    for p, prec in enumerate(("f32", "bf16")):
        for by_chunk in (False, True):
            for i, n in enumerate(ROWS):
                cin, cout = WIDTHS[(i + 2 * p + 3 * by_chunk) % 7]
                K, rpc = OFFSETS[i % 3], RPC[(i + i // 3) % 3]
                cases.append((prec, n, 32 * rpc + 2 if by_chunk else None, rpc, K, cin, cout))
    return cases


def _block_id(case):
    prec, n, cap, rpc, K, cin, cout = case
    return "%s-rows%d-rpc%d-k%d-%dx%d%s" % (prec, n, rpc, K, cin, cout, "-bychunk" if cap else "")


def test_wgrad_block_cases_cover_every_axis():
    """the listed cases hold every value of every axis in both precisions with by_chunk on and off"""
    for prec in ("f32", "bf16"):
        for on in (False, True):
            sel = [c for c in _block_cases() if c[0] == prec and (-(-(c[2] or c[1]) // c[3]) >= 32) == on]
            assert {c[1] for c in sel} == set(ROWS) and {c[3] for c in sel} == set(RPC) and {c[4] for c in sel} == set(OFFSETS)
            assert {(c[5], c[6]) for c in sel} == set(WIDTHS)
            assert all((c[2] is not None) == on for c in sel)


@pytest.mark.parametrize("case", _block_cases(), ids=_block_id)
def test_wgrad_block(device, case):
    prec, n, cap, rpc, K, cin, cout = case
    n_in = n + 5 if n % 2 else max(1, n // 2)
    F, G = operands(n_in, n, cin, cout, seed=n + cin)
    nbr = synthetic_table(n, K, n_in, seed=n + K)
    slabs = run_wgrad_block(device, F, nbr, G, rpc, prec == "bf16", cap, poison=float("nan") if n % 2 else POISON)
    check_wgrad_block(slabs, F, nbr, G, rpc, prec == "bf16")


@pytest.mark.parametrize("prec", ["f32", "bf16"])
@pytest.mark.parametrize("chunks,K,cin,cout", [(31, 27, 64, 64), (32, 27, 64, 64), (33, 8, 130, 62), (39, 27, 66, 130)])
def test_wgrad_block_chunk_counts(device, prec, chunks, K, cin, cout):
    """31 / 32 / 33 / 39 chunks of 32 rows, all rows live: both sides of the by_chunk decode (from 32 chunks on) and chunk
    counts that are no multiple of 8, every chunk's slab checked by value -- a decode that swaps offset and tile, or sends a
    chunk to another XCD's slot, puts a slab where another one belongs"""
    n = 32 * chunks
    F, G = operands(n // 3, n, cin, cout, seed=chunks)
    nbr = synthetic_table(n, K, n // 3, seed=chunks + 1)
    slabs = run_wgrad_block(device, F, nbr, G, 32, prec == "bf16")
    assert slabs.shape[0] == chunks
    check_wgrad_block(slabs, F, nbr, G, 32, prec == "bf16")


@pytest.mark.parametrize("prec", ["f32", "bf16"])
def test_wgrad_block_two_rows_per_chunk(device, prec):
    """rows_per_chunk = 2 (the smallest the entry takes): 17 chunks of one partial 32-row step each, the last of one row"""
    F, G = operands(20, 33, 3, 5, seed=2)
    nbr = synthetic_table(33, 8, 20, seed=3)
    slabs = run_wgrad_block(device, F, nbr, G, 2, prec == "bf16")
    assert slabs.shape[0] == 17
    check_wgrad_block(slabs, F, nbr, G, 2, prec == "bf16")


@pytest.mark.parametrize("prec", ["f32", "bf16"])
@pytest.mark.parametrize("n,cap,rpc,cin,cout", [(33, None, 32, 65, 64), (257, None, 256, 2, 2), (257, 300, 34, 3, 5), (1, None, 32, 1, 1)])
def test_wgrad_block_identity_table(device, prec, n, cap, rpc, cin, cout):
    """nbr == NULL: the identity table of a 1x1x1 convolution (K = 1), exact size and under a capacity"""
    F, G = operands(n, n, cin, cout, seed=n + cout)
    slabs = run_wgrad_block(device, F, None, G, rpc, prec == "bf16", cap)
    check_wgrad_block(slabs, F, None, G, rpc, prec == "bf16")


@pytest.mark.parametrize("prec", ["f32", "bf16"])
@pytest.mark.parametrize("poison", [POISON, float("nan")], ids=["3e38", "nan"])
@pytest.mark.parametrize("live", [0, 1, 299])
@pytest.mark.parametrize("rpc,K,cin,cout", [(32, 27, 64, 64), (256, 8, 3, 5)])
def test_wgrad_block_live_counts(device, prec, poison, live, rpc, K, cin, cout):
    """capacity 300 with a device live count of 0 / 1 / 299 and poison behind it: the slabs of the chunks that hold live rows
    equal the exact-size run on the live rows bit for bit, the others are exactly zero"""
    F, G = operands(120, live, cin, cout, seed=live + K)
    nbr = synthetic_table(live, K, 120, seed=live)
    slabs = run_wgrad_block(device, F, nbr, G, rpc, prec == "bf16", cap=300, poison=poison)
    check_wgrad_block(slabs, F, nbr, G, rpc, prec == "bf16")
    used = -(-live // rpc)
    assert not slabs[used:].any()
    if live:
        exact = run_wgrad_block(device, F, nbr, G, rpc, prec == "bf16")
        assert exact.shape[0] == used and same_bits(slabs[:used], exact)


# ---------------------------------------------------------------------------------------------------------------------
# B. the transposed kernel map
# ---------------------------------------------------------------------------------------------------------------------
def injective_table(n_out, K, n_in, seed, density=0.7):
    """nbr [n_out, K] whose columns are injective (what a kernel map is: for a fixed offset an input has one output)"""
    rng = np.random.RandomState(seed)
    nbr = np.full((n_out, K), -1, dtype=np.int32)
    m = min(n_out, n_in)
    for k in range(K):
        rows, ins = rng.permutation(n_out)[:m], rng.permutation(n_in)[:m]
        keep = rng.rand(m) < density
        nbr[rows[keep], k] = ins[keep]
    return nbr


@pytest.mark.parametrize("no_cap,K,n_in,live", [
    (9, 27, 20, None), (9, 27, 4, None), (32, 8, 50, None), (32, 8, 10, None), (256, 1, 300, None), (256, 1, 100, None),
    (257, 1, 300, None), (257, 1, 100, None), (10, 27, 30, None), (10, 27, 3, None),       # lengths 243 / 256 / 257 / 270
    (9, 27, 20, 5), (32, 8, 50, 20), (32, 8, 10, 31), (257, 1, 300, 129), (10, 27, 30, 1), (256, 1, 100, 200)])
def test_kernel_map_transpose(device, no_cap, K, n_in, live):
    """cnrma_sparse_kernel_map_transpose against numpy: nbr_t[i][k] = the live output row o with nbr[o][k] == i, else -1 (the
    entry fills the table itself: it is handed garbage).  Under a live count the rows behind it are as plausible as the live
    ones (injective, in range) and must not show in nbr_t"""
    from cnrma_amd import sparse as S
    product_library()
    nbr = injective_table(no_cap, K, n_in, seed=no_cap + K + n_in)
    n_live = no_cap if live is None else live
    ref = np.full((n_in, K), -1, dtype=np.int32)
    o, k = np.nonzero(nbr[:n_live] >= 0)
    ref[nbr[o, k], k] = o
    assert (ref == -1).any() and (ref >= 0).any()
    if live is not None:
        assert (nbr[live:] >= 0).any()
    nd = dev(nbr, device)
    no_dev = None if live is None else torch.tensor([live], dtype=torch.int32, device=device)
    outs = []
    for _ in range(2):
        nbr_t = torch.full((n_in, K), 12345, dtype=torch.int32, device=device)
        S.call("cnrma_sparse_kernel_map_transpose", S.ptr(nd), no_cap, S.ptr(no_dev), K, n_in, S.ptr(nbr_t), S.stream())
        outs.append(nbr_t.cpu().numpy())
    assert np.array_equal(outs[0], ref) and np.array_equal(outs[1], ref)
    assert outs[0].max() < n_live


# ---------------------------------------------------------------------------------------------------------------------
# C. the data gradient through conv_autograd
# ---------------------------------------------------------------------------------------------------------------------
def run_autograd(device, c, f, W, ks, stride, ts, prec, seed=0, **switches):
    """conv_autograd forward + backward on exact-size sets under the module switches -> (output coordinates, g, y, dF, dW,
    entries the backward called)"""
    from cnrma_amd import sparse as S
    with settings(**switches):
        st = capacity_tensor(c, f, ts, device)
        x = S.SparseTensor(st.F.detach().requires_grad_(True), st.cs)
        Wd = dev(W, device).requires_grad_(True)
        scrub(device, f.shape, (len(c), W.shape[2]), W.shape)
        y = S.conv_autograd(x, Wd, ks, stride, precision=prec)
        g = np.random.RandomState(seed + 5).randn(*y.F.shape).astype(np.float32)
        with recorded_calls() as seen:
            y.F.backward(dev(g, device))
    return y.C.cpu().numpy().astype(np.int64), g, y.F.detach().cpu().numpy(), x.F.grad.cpu().numpy(), Wd.grad.cpu().numpy(), seen


def check_autograd(device, c, f, W, ks, stride, ts, prec, mirror, go=False):
    """forward, data gradient and weight gradient of one convolution against the fp64 oracle (bf16 entries: on the operands
    they round), twice bit-identical, with the entries of the backward asserted"""
    K, cin, cout = W.shape
    sw = dict(TRAIN_GO=go, WGRAD_GO=False, DGRAD_MIRROR=mirror)
    oc, g, y, dF, dW, seen = run_autograd(device, c, f, W, ks, stride, ts, prec, **sw)
    again = run_autograd(device, c, f, W, ks, stride, ts, prec, **sw)
    assert same_bits(y, again[2]) and same_bits(dF, again[3]) and same_bits(dW, again[4]), "run to run"
    exp_c, exp_y = SO.conv(c, *((bf16_round(f), bf16_round(W)) if prec == "bf16" and cin % 32 == 0 else (f, W)), ks, stride, ts)
    assert np.array_equal(oc, exp_c)
    assert_close(y, exp_y, BF16_BAR if prec == "bf16" and cin % 32 == 0 else F32_BAR, "forward")
    # the data gradient is a convolution of g with Cout input channels: off the 32-multiple it runs in fp32 whatever was asked for
    d16 = prec == "bf16" and cout % 32 == 0
    gF = SO.conv_backward(c, f, bf16_round(W) if d16 else W, bf16_round(g) if d16 else g, ks, stride, ts)[0]
    assert_close(dF, gF, BF16_BAR if d16 else F32_BAR, "data gradient")
    w16 = prec == "bf16"
    gW = SO.conv_backward(c, bf16_round(f) if w16 else f, W, bf16_round(g) if w16 else g, ks, stride, ts)[1]
    assert_close(dW, gW, BF16_BAR if w16 else F32_BAR, "weight gradient")
    transposed = not (mirror and stride == 1 and ks % 2 == 1)
    assert ("cnrma_sparse_kernel_map_transpose" in seen) == transposed, seen
    assert ("cnrma_sparse_conv_wgrad_bf16" if w16 else "cnrma_sparse_conv_wgrad_f32") in seen
    if go:
        assert [n for n in seen if n in CONV_ENTRIES] == ["cnrma_sparse_conv_go_bf16"], seen
    else:
        assert [n for n in seen if n in CONV_ENTRIES] == ["cnrma_sparse_conv_" + (prec if cout % 32 == 0 else "f32")], seen
        assert ("cnrma_sparse_conv_prepare_weights_bf16_t" in seen) == d16, seen
    assert transposed or len(oc) == len(c)
    return oc


COUTS = (1, 3, 33, 65, 96)


def _dgrad_cases():
    """(geometry, precision, Cin, Cout, stride, tensor stride, mirrored form) -- every row count, degenerate set and Cout in
    every precision; stride-1 cases alternate between the mirrored and the transposed-table form, stride 2 is transposed with
    n_in != n_out"""
    cases = []
    geos = [(r, 1, 1) for r in ("rows1", "rows2", "rows63", "rows64", "rows65", "rows129")] + \
        [("lattice", 1, 1), ("twin", 1, 2), ("neg", 2, 2), ("neg", 2, 4), ("neg", 1, 4), ("one_out", 2, 1), ("one_out", 2, 2)]
    for j, prec in enumerate(("f32", "f16x3", "bf16")):
        for i, (geo, stride, ts) in enumerate(geos):
            cases.append((geo, prec, 33 if geo == "lattice" else 32, COUTS[(i + 2 * j) % 5], stride, ts, (i + j) % 2 == 0))
        cases += [("block", prec, 32, 96, 1, 1, True), ("block", prec, 32, 96, 1, 1, False), ("neg", prec, 32, 96, 2, 1, True),
                  ("rows65", prec, 32, 96, 1, 1, j % 2 == 0), ("one_out", prec, 32, 96, 2, 1, True)]
    return cases


def _dgrad_id(case):
    geo, prec, cin, cout, stride, ts, mirror = case
    return "%s-%s-c%d-o%d-s%dt%d-%s" % (prec, geo, cin, cout, stride, ts, "mirrored" if mirror and stride == 1 else "transposed")


def test_data_gradient_cases_cover_every_axis():
    for prec in ("f32", "f16x3", "bf16"):
        sel = [c for c in _dgrad_cases() if c[1] == prec]
        assert {c[3] for c in sel} == set(COUTS)
        assert {c[0] for c in sel} >= {"rows1", "rows2", "rows63", "rows64", "rows65", "rows129", "lattice", "twin", "neg", "one_out"}
        for form in (True, False):           # both forms at the width that keeps the asked-for precision and at one that does not
            assert {c[3] % 32 == 0 for c in sel if c[4] == 1 and c[6] == form} == {True, False}
        assert any(c[4] == 2 and c[3] == 96 for c in sel)


@pytest.mark.parametrize("case", _dgrad_cases(), ids=_dgrad_id)
def test_data_gradient(device, case):
    geo, prec, cin, cout, stride, ts, mirror = case
    c = GEOMETRY[geo](ts)
    oc = check_autograd(device, c, features(len(c), cin), weights(27, cin, cout), 3, stride, ts, prec, mirror)
    if geo == "one_out":
        assert len(oc) == 1                                # every input row shares one parent
    if stride == 2:
        assert len(oc) != len(c)


@pytest.mark.parametrize("geo,cin,cout", [("block", 64, 64), ("rows65", 96, 64), ("rows1", 64, 96)])
def test_data_gradient_on_the_gather_once_kernel(device, geo, cin, cout):
    """TRAIN_GO = True: forward and mirrored data gradient of the bf16 step on cnrma_sparse_conv_go_bf16 at a few rows"""
    c = GEOMETRY[geo](1)
    check_autograd(device, c, features(len(c), cin), weights(27, cin, cout), 3, 1, 1, "bf16", True, go=True)


@pytest.mark.parametrize("prec", ["f32", "bf16"])
def test_data_gradient_of_a_1x1x1_convolution(device, prec):
    """kernel size 1: no table at all (nbr None on both sides), weights transposed"""
    c = block(65, lo=-2)
    from cnrma_amd import sparse as S
    f, W = features(65, 32), weights(1, 32, 96)[0]
    with settings(TRAIN_GO=False, WGRAD_GO=False):
        x = S.SparseTensor(dev(f, device).requires_grad_(True), capacity_tensor(c, f, 1, device).cs)
        Wd = dev(W, device).requires_grad_(True)
        y = S.conv_autograd(x, Wd, 1, 1, precision=prec)
        g = features(65, 96, seed=3)
        with recorded_calls() as seen:
            y.F.backward(dev(g, device))
    assert "cnrma_sparse_kernel_map_transpose" not in seen
    b16 = prec == "bf16"
    r = bf16_round if b16 else (lambda a: a)
    bar = BF16_BAR if b16 else F32_BAR
    assert_close(x.F.grad.cpu().numpy(), r(g).astype(np.float64) @ r(W).astype(np.float64).T, bar, "data gradient")
    assert_close(Wd.grad.cpu().numpy(), r(f).astype(np.float64).T @ r(g).astype(np.float64), bar, "weight gradient")


# ---------------------------------------------------------------------------------------------------------------------
# D. weight gradient, gather-once kernel
# ---------------------------------------------------------------------------------------------------------------------
GO_HDR = 84           # ints per tile at the head of the tile-union buffer: [0] groups, then {offset mask, first entry, entries} each


def ordered_rows(device, n, order, cin, seed=0):
    """(coordinates, features) of n rows: "morton" = the voxeliser's compact Morton order (one offset group per tile),
    "shuffled" = a dense cube in random row order (tiles without locality: several groups)"""
    from cnrma_amd import sparse as S
    f = features(n, cin, seed)
    if order == "shuffled":
        return block(n, lo=-3, seed=seed), f
    pts = block(n, lo=-3, seed=seed)[:, 1:].astype(np.float32) + 0.5
    st, _ = S.voxelize(torch.from_numpy(pts).to(device), torch.from_numpy(f).to(device), 1.0)
    assert st.cs.n == n and st.cs.compact
    return st.C.cpu().numpy().astype(np.int64), st.F.cpu().numpy()


def run_wgrad_go(device, c, f, g, parts, cap=None, compact=False, poison=POISON):
    """cnrma_sparse_conv_wgrad_go_bf16 on tile_union(...) of the set (c, capacity `cap`, the union built with the same live
    word), NaN-prefilled slabs, twice -> (slabs [parts, 27, Cin, Cout], the live rows of the neighbour table, tile headers)"""
    from cnrma_amd import sparse as S
    product_library()
    live, cin = f.shape
    cout = g.shape[1]
    x = capacity_tensor(c, f, 1, device, cap, poison, compact=compact)
    cs = x.cs
    assert (cs.n_dev is None) == (cap is None or cap == live)
    tu = S.tile_union(cs, cs, 3, 1)
    nbr = cs.neighbours(cs, 3, 1).cpu().numpy()[:live]
    assert nbr.max() < live and nbr.min() >= -1
    tiles = -(-cs.n // 64)
    hdr = tu[:tiles * GO_HDR * 4].view(torch.int32).view(tiles, GO_HDR).cpu().numpy()
    Gd = poison_rows(g, cs.n, device, poison) if cs.n > live else dev(g, device)
    outs = []
    for _ in range(2):
        slabs = torch.full((parts, 27, cin, cout), float("nan"), dtype=torch.float32, device=device)
        S.call("cnrma_sparse_conv_wgrad_go_bf16", S.ptr(x.F), cin, S.ptr(tu), S.ptr(Gd), cout, cs.n, S.ptr(cs.n_dev), parts,
               S.ptr(slabs), S.stream())
        outs.append(slabs.cpu().numpy())
    assert not np.isnan(outs[0]).any(), "an element of a slab was not written"
    assert same_bits(outs[0], outs[1]), "run to run"
    return outs[0], nbr, hdr


def check_wgrad_go(device, c, f, g, cap=None, compact=False, poison=POISON, parts_list=None):
    """parts = 1, the number of tiles, 16 and 17: every part's slab against fp64 on the part's live rows (bf16-rounded
    operands), a part without live tiles exactly zero; the sum against the oracle's conv_backward (its own neighbour search)
    and against the block kernel on the same operands -> the tile headers"""
    live = len(f)
    tiles_cap = -(-(cap or live) // 64)
    Fo, Go = bf16_round(f), bf16_round(g)
    gW = SO.conv_backward(c, Fo, np.zeros((27, f.shape[1], g.shape[1])), Go, 3, 1, 1)[1]
    blk = None
    for parts in parts_list or sorted({1, tiles_cap, 16, 17}):
        slabs, nbr, hdr = run_wgrad_go(device, c, f, g, parts, cap, compact, poison)
        per = -(-tiles_cap // parts) * 64
        empty = 0
        for p in range(parts):
            r0, r1 = p * per, min(live, (p + 1) * per)
            if r0 >= live:
                assert not slabs[p].any(), "part %d of %d has no live tile" % (p, parts)
                empty += 1
            else:
                assert_close(slabs[p], wgrad_ref(Fo, nbr, Go, r0, r1), BF16_BAR, "part %d of %d" % (p, parts))
        assert parts < 16 or empty > 0
        total = slabs.astype(np.float64).sum(0)
        assert_close(total, gW, BF16_BAR, "sum of %d parts" % parts)
        if blk is None:
            blk = run_wgrad_block(device, f, nbr, g, 256, True).astype(np.float64).sum(0)
        assert np.abs(total - blk).max() <= BF16_BAR * np.abs(blk).max()
    return hdr, nbr


GO_WIDTHS = ((4, 4), (36, 20), (64, 64), (68, 132), (132, 68))


@pytest.mark.parametrize("order", ["morton", "shuffled"])
@pytest.mark.parametrize("i,n", list(enumerate((1, 63, 64, 65, 129, 257))))
def test_wgrad_go_direct(device, order, i, n):
    """1 / 63 / 64 / 65 / 129 / 257 rows (the Python switch keeps the kernel from fewer than 256), Morton rows and shuffled
    rows, every width once per order; parts 1, the number of tiles, 16 and 17 (by_part decode, trailing parts without a tile)"""
    cin, cout = GO_WIDTHS[(i + 2 * (order == "shuffled")) % 5]
    c, f = ordered_rows(device, n, order, cin)
    g = features(n, cout, seed=9)
    hdr, nbr = check_wgrad_go(device, c, f, g, compact=order == "morton")
    tiles = -(-n // 64)
    groups = hdr[:tiles, 0]
    assert (groups >= 1).all()
    if order == "morton":
        assert (groups == 1).all()
        counts = [len(np.unique(t[t >= 0])) for t in (nbr[64 * t0:64 * t0 + 64] for t0 in range(tiles))]
        assert (hdr[:tiles, 3] == counts).all()                        # a one-group tile's union = its distinct input rows
        if n in (1, 63):
            assert counts[-1] % 2 == 1                                 # an odd union count: the last row pair is half empty


@pytest.mark.parametrize("cin,cout", [(64, 64), (36, 20)])
def test_wgrad_go_partial_tile_with_several_groups(device, cin, cout):
    """370 shuffled rows of an 8^3 cube: the last tile has 50 rows whose neighbourhoods cover most of the cube -- more than the
    280 rows of one union image, so the PARTIAL tile is staged in place over several offset groups"""
    c, f = ordered_rows(device, 370, "shuffled", cin)
    hdr, _ = check_wgrad_go(device, c, f, features(370, cout, seed=9), parts_list=(1, 6, 16, 17))
    assert 370 % 64 == 50 and hdr[5, 0] > 1
    counts = np.concatenate([hdr[t, 3:3 + 3 * hdr[t, 0]:3] for t in range(6)])
    assert (counts % 2 == 1).any() and (counts <= 280).all()


@pytest.mark.parametrize("order", ["morton", "shuffled"])
@pytest.mark.parametrize("poison", [POISON, float("nan")], ids=["3e38", "nan"])
def test_wgrad_go_capacity(device, order, poison):
    """129 live rows under a capacity of 300 (5 tiles, 3 of them live), the union built with the same live word; coordinates,
    features and gradient rows behind the live count are poison.  Parts of dead tiles are exactly zero and the parts that hold
    live rows equal the exact-size run bit for bit"""
    cin, cout = (64, 64) if order == "morton" else (36, 20)
    c, f = ordered_rows(device, 129, order, cin)
    g = features(129, cout, seed=9)
    check_wgrad_go(device, c, f, g, cap=300, compact=order == "morton", poison=poison)
    capped = run_wgrad_go(device, c, f, g, 5, 300, order == "morton", poison)[0]
    exact = run_wgrad_go(device, c, f, g, 3, None, order == "morton")[0]
    assert same_bits(capped[:3], exact) and not capped[3:].any()


@pytest.mark.parametrize("n,order,cin,cout", [(63, "shuffled", 36, 20), (257, "morton", 64, 64), (129, "shuffled", 68, 132)])
def test_wgrad_go_through_autograd(device, n, order, cin, cout):
    """WGRAD_GO = True: the bf16 backward of conv_autograd takes the gather-once weight gradient (parts chosen by Python) below
    WGRAD_GO_MIN_ROWS too; against the fp64 oracle on rounded operands"""
    c, f = ordered_rows(device, n, order, cin)
    W = weights(27, cin, cout)
    oc, g, _, _, dW, seen = run_autograd(device, c, f, W, 3, 1, 1, "bf16", TRAIN_GO=False, WGRAD_GO=True, DGRAD_MIRROR=True)
    assert "cnrma_sparse_conv_wgrad_go_bf16" in seen and "cnrma_sparse_conv_wgrad_bf16" not in seen
    assert_close(dW, SO.conv_backward(c, bf16_round(f), W, bf16_round(g), 3, 1, 1)[1], BF16_BAR, "weight gradient")


# ---------------------------------------------------------------------------------------------------------------------
# E. BatchNorm training kernels
# ---------------------------------------------------------------------------------------------------------------------
ACTS = {None: False, "relu": True, "elu": "elu"}
CONSTANT, OFFSET = 1, 2         # columns of every input with more than 3 rows and 4 columns: a constant, and 1000 + 0.01 randn


def bn_inputs(n, C, act, with_res, seed):
    rng = np.random.RandomState(seed)
    x = (rng.randn(n, C) * 3 + 1.5).astype(np.float32)
    special = n > 3 and C >= 4
    if special:
        x[:, CONSTANT] = 2.5
        x[:, OFFSET] = (1000 + 0.01 * rng.randn(n)).astype(np.float32)
    w = rng.uniform(0.5, 1.5, C).astype(np.float32)
    b = rng.randn(C).astype(np.float32)
    r = rng.randn(n, C).astype(np.float32) if with_res else None
    g = rng.randn(n, C).astype(np.float32)
    x, b, r = clear_of_kink(x, w, b, EPS, r, act)
    if act is not None:
        assert np.abs(SO.batch_norm_train(x, w, b, EPS, r, act)[1]["pre"]).min() >= 0.04        # fp64, on the CPU: no element near the kink
    classes = {"ordinary": np.array([j for j in range(C) if not special or j not in (CONSTANT, OFFSET)])}
    if special:
        classes.update(constant=np.array([CONSTANT]), offset=np.array([OFFSET]))
    return x, w, b, r, g, classes


def bn_module(C, w, b, device):
    bn = torch.nn.BatchNorm1d(C, eps=EPS, momentum=0.1).to(device).train()
    with torch.no_grad():
        bn.weight.copy_(torch.from_numpy(w))
        bn.bias.copy_(torch.from_numpy(b))
    return bn


def bn_through(fn, bn, x, r, g, act, device):
    """forward + backward of act(fn(x) [+ r]) -> dict of numpy outputs"""
    xd = dev(x, device).requires_grad_(True)
    rd = dev(r, device).requires_grad_(True) if r is not None else None
    y = fn(xd, rd)
    y.backward(dev(g, device))
    out = dict(y=y.detach(), dx=xd.grad, dw=bn.weight.grad, db=bn.bias.grad, running_mean=bn.running_mean, running_var=bn.running_var)
    if r is not None:
        out["dres"] = rd.grad
    assert int(bn.num_batches_tracked) == 1
    return {k: v.cpu().numpy() for k, v in out.items()}


def bn_reference(x, w, b, r, g, act):
    n = x.shape[0]
    y, st = SO.batch_norm_train(x, w, b, EPS, r, act)
    dx, dres, dw, db = SO.batch_norm_train_backward(x, w, b, EPS, g, r, act)
    ref = dict(y=y, dx=dx, dw=dw, db=db, running_mean=0.1 * st["mean"], running_var=0.9 + 0.1 * st["var"] * n / (n - 1))
    if r is not None:
        ref["dres"] = dres
    return ref


def bn_bars(got, tor, ref, classes, label):
    """per output and column class: the kernel's error against fp64 <= max(4 x torch's error against fp64, 1e-6 max|ref|);
    every figure is printed before it is asserted"""
    bad = []
    for name in sorted(ref):
        for cls, cols in classes.items():
            e_k = float(np.abs(got[name][..., cols] - ref[name][..., cols]).max())
            e_t = float(np.abs(tor[name][..., cols] - ref[name][..., cols]).max())
            scale = float(np.abs(ref[name][..., cols]).max())
            bar = max(4 * e_t, 1e-6 * scale)
            print("%s %-12s %-8s kernel %.3e torch %.3e max|ref| %.3e bar %.3e" % (label, name, cls, e_k, e_t, scale, bar))
            if not e_k <= bar:
                bad.append((name, cls, e_k, bar))
    assert not bad, bad


def run_bn_train(device, n, C, act, with_res, seed):
    from cnrma_amd import sparse as S
    x, w, b, r, g, classes = bn_inputs(n, C, act, with_res, seed)
    ref = bn_reference(x, w, b, r, g, act)
    torch_bn, hip_bn = bn_module(C, w, b, device), bn_module(C, w, b, device)

    def composed(xd, rd):
        y = torch_bn(xd)
        y = y + rd if rd is not None else y
        return torch.relu(y) if act == "relu" else (torch.nn.functional.elu(y) if act == "elu" else y)
    scrub(device, x.shape, (C,))
    with settings(BN_TRAIN_HIP=True), recorded_calls() as seen:
        got = bn_through(lambda xd, rd: S.batch_norm_train(xd, hip_bn, relu=ACTS[act], residual=rd), hip_bn, x, r, g, act, device)
    assert seen == ["cnrma_bn_train_forward_f32", "cnrma_bn_train_backward_f32"]
    tor = bn_through(composed, torch_bn, x, r, g, act, device)
    bn_bars(got, tor, ref, classes, "n%d c%d %s%s" % (n, C, act, "+res" if with_res else ""))
    o = classes["ordinary"]                     # the tolerances of test_batch_norm_train_kernels_match_torch, nothing masked
    np.testing.assert_allclose(got["y"][:, o], tor["y"][:, o], rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(got["dx"][:, o], tor["dx"][:, o], rtol=1e-3, atol=2e-5)
    if with_res:
        np.testing.assert_allclose(got["dres"][:, o], tor["dres"][:, o], rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(got["dw"][o], tor["dw"][o], rtol=1e-3, atol=1e-3)
    np.testing.assert_allclose(got["db"][o], tor["db"][o], rtol=1e-3, atol=1e-3)
    np.testing.assert_allclose(got["running_mean"][o], tor["running_mean"][o], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(got["running_var"][o], tor["running_var"][o], rtol=1e-4, atol=1e-6)
    return got, ref


BN_ROWS = (2, 3, 255, 257, 1025)
BN_WIDTHS = (4, 36, 100, 252, 256)


def _bn_cases():
    """every act x residual combination at every row count, the widths rotated: all 25 (n, C) pairs but five appear"""
    cases = []
    for j, (act, with_res) in enumerate(itertools.product((None, "relu", "elu"), (False, True))):
        for i, n in enumerate(BN_ROWS):
            cases.append((n, BN_WIDTHS[(i + j) % 5], act, with_res))
    return cases


@pytest.mark.parametrize("n,C,act,with_res", _bn_cases(),
                         ids=["n%d-c%d-%s-%s" % (n, C, act or "none", "res" if r else "nores") for n, C, act, r in _bn_cases()])
def test_bn_train(device, n, C, act, with_res):
    """cnrma_bn_train_forward_f32 / _backward_f32 against fp64: n = 2 .. 1025, widths that leave idle threads in the column-sum
    kernel (256 % C != 0), all six act x residual combinations, a constant column and a column of 1000 + 0.01 randn"""
    got, ref = run_bn_train(device, n, C, act, with_res, seed=n + C)
    if n == 2:          # the unbiased estimate of two rows is twice the biased one
        x = bn_inputs(n, C, act, with_res, n + C)[0].astype(np.float64)
        np.testing.assert_allclose(ref["running_var"], 0.9 + 0.1 * 2 * x.var(0), rtol=1e-12)
        np.testing.assert_allclose(got["running_var"], 0.9 + 0.1 * 2 * x.var(0), rtol=1e-6)


@pytest.mark.parametrize("act,with_res", [("relu", True), (None, False)])
def test_bn_train_grid_stride(device, act, with_res):
    """n * C / 4 = 1 049 600 items > 256 * 4096 threads: the grid-stride loops of the apply kernels take a second turn"""
    assert 16400 * 256 // 4 > 256 * 4096
    run_bn_train(device, 16400, 256, act, with_res, seed=1)


@pytest.mark.parametrize("n,C,gain", [(2, 1, True), (257, 3, True), (1025, 5, True), (3, 36, True), (255, 255, True), (1025, 256, True),
                                      (257, 5, False)])
def test_bn_backward_any_width(device, n, C, gain):
    """cnrma_bn_backward_f32 (the scalar backward for any C; nothing called it before) through the C ABI, its statistics from
    cnrma_sparse_instnorm_f32 as its comment prescribes; same reference and bars as the fused kernels"""
    from cnrma_amd import sparse as S
    lib = product_library()
    x, w, b, _, g, classes = bn_inputs(n, C, None, False, seed=3 * n + C)
    if not gain:
        w = np.ones_like(w)
    ref = {k: v for k, v in bn_reference(x, w, b, None, g, None).items() if k in ("dx", "dw", "db")}
    st = SO.batch_norm_train(x, w, b, EPS)[1]
    torch_bn = bn_module(C, w, b, device)
    tor = bn_through(lambda xd, rd: torch_bn(xd), torch_bn, x, None, g, None, device)
    words = lib.cnrma_instnorm_workspace_bytes(C) // 8
    stats = torch.full((words,), float("nan"), dtype=torch.float64, device=device)
    ws = torch.full((words,), float("nan"), dtype=torch.float64, device=device)
    xd, gd, wd = dev(x, device), dev(g, device), dev(w, device)
    outs = []
    for _ in range(2):
        dx = torch.full((n, C), float("nan"), dtype=torch.float32, device=device)
        dw, db = (torch.full((C,), float("nan"), dtype=torch.float32, device=device) for _ in range(2))
        S.call("cnrma_sparse_instnorm_f32", S.ptr(xd), n, None, None, C, None, None, EPS, 0, None, S.ptr(stats), S.stream())
        S.call("cnrma_bn_backward_f32", S.ptr(gd), S.ptr(xd), n, C, S.ptr(stats), S.ptr(wd) if gain else None, EPS,
               S.ptr(dx), S.ptr(dw), S.ptr(db), S.ptr(ws), S.stream())
        outs.append(dict(dx=dx.cpu().numpy(), dw=dw.cpu().numpy(), db=db.cpu().numpy()))
    for k in ref:
        assert same_bits(outs[0][k], outs[1][k]) and not np.isnan(outs[0][k]).any()
    # fp64 sums of at most 1025 fp32 values: the statistics carry a few roundings of 2^-53 relative to mean^2 + var
    mean, var = stats[:C].cpu().numpy(), stats[C:2 * C].cpu().numpy()
    assert (np.abs(mean - st["mean"]) <= 1e-12 * np.maximum(1, np.abs(st["mean"]))).all()
    assert (np.abs(var - st["var"]) <= 1e-12 * (st["mean"] ** 2 + st["var"])).all()
    bn_bars(outs[0], tor, ref, classes, "n%d c%d any-width" % (n, C))


# ---------------------------------------------------------------------------------------------------------------------
# F. composites
# ---------------------------------------------------------------------------------------------------------------------
def pool_case(device, c, f, ts, relu_first=False):
    """S.max_pool (behind a ReLU if asked) forward + backward -> (input gradient, pooled rows, oracle gradient, oracle rows)"""
    from cnrma_amd import sparse as S
    cs = capacity_tensor(c, f, ts, device).cs
    fd = dev(f, device).requires_grad_(True)
    scrub(device, f.shape)
    with recorded_calls() as seen:
        y = S.max_pool(S.SparseTensor(torch.relu(fd) if relu_first else fd, cs))
        g = np.random.RandomState(len(c)).randn(*y.F.shape).astype(np.float32)
        y.F.backward(dev(g, device))
    assert "cnrma_sparse_maxpool_f32" in seen and "cnrma_sparse_kernel_map_transpose" in seen
    fin = np.maximum(f, 0) if relu_first else f
    oc, out = SO.max_pool(c, fin, ts)
    assert np.array_equal(y.C.cpu().numpy().astype(np.int64), oc)
    assert np.array_equal(y.F.detach().cpu().numpy().astype(np.float64), out)
    gF = SO.max_pool_backward(c, fin, g, ts)
    if relu_first:
        gF = gF * (f > 0)
    return fd.grad.cpu().numpy(), gF, oc


POOL_GEOMETRY = [("rows1", 1), ("rows2", 1), ("rows63", 2), ("rows64", 1), ("rows65", 1), ("rows129", 2), ("lattice", 1), ("neg", 2),
                 ("neg", 4), ("one_out", 1), ("twin", 1)]


@pytest.mark.parametrize("geo,ts", POOL_GEOMETRY, ids=["%s-t%d" % g for g in POOL_GEOMETRY])
@pytest.mark.parametrize("C", [1, 5, 32])
def test_max_pool_gradient(device, geo, ts, C):
    """_MaxPoolFn.backward by value: the gradient of a parent goes to the child that attains the maximum, every other child
    gets exactly zero -- exact (a gather of fp32 values), on 1 to 300 input rows, isolated rows and negative coordinates"""
    c = GEOMETRY[geo](ts)
    f = features(len(c), C, seed=4)
    got, gF, oc = pool_case(device, c, f, ts)
    look = SO.Lookup(oc)                                                          # distinct values per window and channel
    parent = look(np.concatenate((c[:, :1], c[:, 1:] // (2 * ts) * (2 * ts)), axis=1))
    for p in np.unique(parent):
        rows = f[parent == p]
        assert (np.sort(rows, axis=0)[1:] != np.sort(rows, axis=0)[:-1]).all()
    assert np.array_equal(got.astype(np.float64), gF)
    assert (np.count_nonzero(gF, axis=0) == len(oc)).all()


@pytest.mark.parametrize("geo,ts", [("rows129", 1), ("neg", 2), ("lattice", 1)])
def test_relu_max_pool_gradient(device, geo, ts):
    """a ReLU in front: half of the candidates are tied zeros.  Where the window's maximum is positive it is unique; where it is
    0 the pooling marks every tied child and the ReLU's own backward zeroes them all -- the composition has one answer"""
    c = GEOMETRY[geo](ts)
    f = features(len(c), 8, seed=6)
    got, gF, _ = pool_case(device, c, f, ts, relu_first=True)
    assert (f <= 0).mean() > 0.3
    assert np.array_equal(got.astype(np.float64), gF)


FUSED_BAR = 2e-5


def fused_node(device, c, f, W, w, b, res, g, stride, ts, act, prec, fuse=True):
    """conv_bn_act_train forward + backward -> dict of numpy outputs, the entries called, the output coordinates"""
    from cnrma_amd import sparse as S
    cout = W.shape[2]
    with settings(FUSE_CONV_BN=fuse, BN_TRAIN_HIP=True, TRAIN_GO=False, WGRAD_GO=False, DGRAD_MIRROR=True):
        st = capacity_tensor(c, f, ts, device)
        x = S.SparseTensor(st.F.detach().requires_grad_(True), st.cs)
        Wd = dev(W, device).requires_grad_(True)
        bn = bn_module(cout, w, b, device)
        out_cs = st.cs if stride == 1 else st.cs.strided(2)
        rd = dev(res, device).requires_grad_(True) if res is not None else None
        scrub(device, f.shape, g.shape, W.shape, (cout,))
        with recorded_calls() as seen:
            y = S.conv_bn_act_train(x, Wd, bn, 3, stride, act, None if rd is None else S.SparseTensor(rd, out_cs), precision=prec)
            y.F.backward(dev(g, device))
    out = dict(y=y.F.detach(), dF=x.F.grad, dW=Wd.grad, dw=bn.weight.grad, db=bn.bias.grad, running_mean=bn.running_mean,
               running_var=bn.running_var)
    if rd is not None:
        out["dres"] = rd.grad
    return {k: v.cpu().numpy() for k, v in out.items()}, seen, y.C.cpu().numpy().astype(np.int64)


def fused_reference(c, f, W, w, b, res, g, stride, ts, act):
    """the fp64 composition: oracle convolution -> BatchNorm reference -> their backwards"""
    oc, y0 = SO.conv(c, f, W, 3, stride, ts)
    n = len(oc)
    y, st = SO.batch_norm_train(y0, w, b, EPS, res, act)
    dx, dres, dw, db = SO.batch_norm_train_backward(y0, w, b, EPS, g, res, act)
    dF, dW = SO.conv_backward(c, f, W, dx, 3, stride, ts)
    ref = dict(y=y, dF=dF, dW=dW, dw=dw, db=db, running_mean=0.1 * st["mean"], running_var=0.9 + 0.1 * st["var"] * n / (n - 1))
    if res is not None:
        ref["dres"] = dres
    return ref, st["pre"]


@pytest.mark.parametrize("geo,cin,cout,stride,act,with_res", [("block", 64, 64, 1, "relu", True), ("neg", 32, 64, 2, "elu", False)])
def test_fused_conv_bn_act(device, geo, cin, cout, stride, act, with_res):
    """conv_bn_act_train as ONE autograd node (f32) against the fp64 composition, and bit for bit against its unfused form
    (conv_autograd + batch_norm_train: the same kernels in the same order).
    Bar 2e-5 max|ref| per output: the stages are fp32-grade one by one (convolution 2e-6 max|y0|, BatchNorm ~1e-6), but the
    BatchNorm divides the convolution's error by sigma: with max|y0| about 4 sigma over 300 rows and a gain of up to 1.5 that
    is 2e-6 x 4 x 1.5 = 1.2e-5 of an output of order one, and the backward passes the same factor once more into a gradient
    whose largest element is several times its typical one.
    ReLU: the residual keeps every pre-activation 0.04 away from the kink; ELU without a residual has nothing to move and needs
    nothing: its slope (y + 1 below zero, 1 above) is continuous, so a rounding across 0 changes the gradient by that rounding"""
    c = GEOMETRY[geo](1)
    f, W = features(len(c), cin), weights(27, cin, cout)
    rng = np.random.RandomState(cin + cout)
    w, b = rng.uniform(0.5, 1.5, cout).astype(np.float32), rng.randn(cout).astype(np.float32)
    oc, y0 = SO.conv(c, f, W, 3, stride, 1)
    res = rng.randn(len(oc), cout).astype(np.float32) if with_res else None
    _, b, res = clear_of_kink(y0, w, b, EPS, res, act if with_res else None)
    g = rng.randn(len(oc), cout).astype(np.float32)
    ref, pre = fused_reference(c, f, W, w, b, res, g, stride, 1, act)
    assert act != "relu" or np.abs(pre).min() >= 0.04
    got, seen, out_c = fused_node(device, c, f, W, w, b, res, g, stride, 1, act, "f32")
    assert np.array_equal(out_c, oc)
    assert "cnrma_bn_train_forward_f32" in seen and "cnrma_bn_train_backward_f32" in seen and "cnrma_sparse_conv_wgrad_f32" in seen
    for k in sorted(ref):
        err = float(np.abs(got[k] - ref[k]).max())
        print("%-12s error %.3e of max|ref| %.3e = %.2e" % (k, err, np.abs(ref[k]).max(), err / np.abs(ref[k]).max()))
    for k in sorted(ref):
        assert_close(got[k], ref[k], FUSED_BAR, k)
    unfused, seen2, _ = fused_node(device, c, f, W, w, b, res, g, stride, 1, act, "f32", fuse=False)
    assert [n for n in seen2 if n.startswith("cnrma_bn_")] == ["cnrma_bn_train_forward_f32", "cnrma_bn_train_backward_f32"]
    for k in sorted(ref):
        assert same_bits(got[k], unfused[k]), k


def test_fused_conv_bn_act_fallbacks(device):
    """where the fused node does not apply it composes conv_autograd with batch_norm_train: Cout = 260 (wider than the fused
    BatchNorm's 256 columns: torch's BatchNorm behind the HIP convolution) against the fp64 composition; one output row
    (a batch statistic of one row does not exist): no BatchNorm kernel runs and torch's own refusal comes through"""
    c = GEOMETRY["rows65"](1)
    f, W = features(65, 32), weights(27, 32, 260)
    rng = np.random.RandomState(260)
    w, b = rng.uniform(0.5, 1.5, 260).astype(np.float32), rng.randn(260).astype(np.float32)
    y0 = SO.conv(c, f, W, 3, 1, 1)[1]
    res = rng.randn(65, 260).astype(np.float32)
    _, b, res = clear_of_kink(y0, w, b, EPS, res, "relu")
    g = rng.randn(65, 260).astype(np.float32)
    ref, pre = fused_reference(c, f, W, w, b, res, g, 1, 1, "relu")
    assert np.abs(pre).min() >= 0.04
    got, seen, _ = fused_node(device, c, f, W, w, b, res, g, 1, 1, "relu", "f32")
    assert not [n for n in seen if n.startswith("cnrma_bn_")] and "cnrma_sparse_conv_f32" in seen
    for k in sorted(ref):
        assert_close(got[k], ref[k], FUSED_BAR, k)
    c = GEOMETRY["one_out"](1)
    f, W = features(len(c), 32), weights(27, 32, 64)
    w, b = np.ones(64, dtype=np.float32), np.zeros(64, dtype=np.float32)
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        fused_node(device, c, f, W, w, b, None, np.ones((1, 64), dtype=np.float32), 2, 1, "relu", "f32")


# ---------------------------------------------------------------------------------------------------------------------
# refused arguments: every one of them returns before a launch
# ---------------------------------------------------------------------------------------------------------------------
def test_refused_arguments(device):
    from cnrma_amd import _lib
    from cnrma_amd import sparse as S
    lib = product_library()
    F, G = dev(features(8, 6), device), dev(features(8, 6, seed=1), device)
    nbr = dev(synthetic_table(8, 27, 8, 0), device)
    slabs = torch.zeros((8, 27, 6, 6), dtype=torch.float32, device=device)
    for entry in ("cnrma_sparse_conv_wgrad_f32", "cnrma_sparse_conv_wgrad_bf16"):
        with pytest.raises(_lib.CnrmaError):          # an odd rows_per_chunk
            S.call(entry, S.ptr(F), 6, S.ptr(nbr), 27, S.ptr(G), 6, 8, None, 3, S.ptr(slabs), S.stream())
    cs = capacity_tensor(block(8), features(8, 6), 1, device).cs
    with pytest.raises(_lib.CnrmaError):              # Cin % 4 != 0 for the gather-once weight gradient
        S.call("cnrma_sparse_conv_wgrad_go_bf16", S.ptr(F), 6, S.ptr(S.tile_union(cs, cs, 3, 1)), S.ptr(G), 6, 8, None, 1, S.ptr(slabs),
               S.stream())
    x = dev(features(1, 4), device)
    ws = torch.zeros(lib.cnrma_instnorm_workspace_bytes(4) // 8, dtype=torch.float64, device=device)
    with pytest.raises(_lib.CnrmaError):              # a batch statistic needs two rows
        S.call("cnrma_bn_train_forward_f32", S.ptr(x), 1, 4, None, None, EPS, None, 0, 0.1, None, None, None, S.ptr(torch.empty_like(x)),
               S.ptr(ws), S.stream())
    assert not slabs.any()
