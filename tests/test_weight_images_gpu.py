"""GPU tests (-m gpu) of the prepared weight images (csrc/sparse.hip "Prepared weight images"): each of the eight prepare entry
points is compared BYTE FOR BYTE with the exact host oracle (oracle/sparse_oracle.py weight_image) -- the encodings are
reproducible bit for bit on the CPU, so nothing here has a tolerance.

Shapes (K, Cin, Cout), the smallest that can still go wrong:
  (1, 32, 4)      one slice; one 32-column tile live, the other three column tiles all padding
  (3, 64, 130)    two slices; padding to 256 crosses a 128 boundary; a partial last column tile
  (2, 12, 20)     stage-order kinds only: the plain [K][Cout_p][Cin] branch
  (3, 32, 64), (3, 64, 32) with flip 0 / 1: the transposed images (K = 3 separates mirrored from plain with a fixed centre,
                  Cin != Cout catches a swapped transpose)
  (27, 256, 256)  the only one whose element count exceeds the block cap times 256 (1.77 M > 1.05 M; the pair 3.5 M > 2.1 M):
                  the grid-stride step actually runs
W is random normal with distinct values; the fp16 trailer equals max|W| exactly (the bound is found without arithmetic)."""
import functools

import numpy as np
import pytest
import torch

from oracle import sparse_oracle as SO

pytestmark = pytest.mark.gpu

# kind -> (bytes query, prepare entry point)
ENTRY = {
    "bf16x3": ("cnrma_sparse_conv_weight_bytes", "cnrma_sparse_conv_prepare_weights"),
    "f16": ("cnrma_sparse_conv_f16_weight_bytes", "cnrma_sparse_conv_prepare_weights_f16"),
    "bf16": ("cnrma_sparse_conv_bf16_weight_bytes", "cnrma_sparse_conv_prepare_weights_bf16"),
    "f16_frag": ("cnrma_sparse_conv_f16_weight_bytes", "cnrma_sparse_conv_prepare_weights_f16_frag"),
    "f32_frag": ("cnrma_sparse_conv_f32_frag_weight_bytes", "cnrma_sparse_conv_prepare_weights_f32_frag"),
    "bf16_frag": ("cnrma_sparse_conv_bf16_frag_weight_bytes", "cnrma_sparse_conv_prepare_weights_bf16_frag"),
}
STAGE_KINDS = ("bf16x3", "f16", "bf16")
FP16_KINDS = ("f16", "f16_frag")


@functools.lru_cache(maxsize=None)
def _weights(shape):
    """random normal fp32 [K, Cin, Cout], all values distinct; made once per shape and never modified"""
    n = int(np.prod(shape))
    rng = np.random.default_rng(1000 + n)
    v = np.unique(rng.standard_normal(2 * n + 16).astype(np.float32))
    assert len(v) >= n
    W = rng.permutation(v)[:n].reshape(shape)
    W.setflags(write=False)
    return W


@functools.lru_cache(maxsize=None)
def _expected(kind, shape, transpose=False, flip=False):
    return SO.weight_image(kind, _weights(shape), transpose=transpose, flip=flip)


def _buffer(query, K, Ci, Co):
    from cnrma_amd import _lib
    return torch.full((getattr(_lib.load(), query)(K, Ci, Co),), 0xA5, dtype=torch.uint8, device="cuda")


def _prepare(kind, W, *args, transposed=False, entry=None):
    """the image of W through `entry` (default: the kind's own) as host bytes; args sit between Cout and the image"""
    from cnrma_amd._lib import call, ptr, stream
    K, Cin, Cout = W.shape
    w = torch.tensor(W, device="cuda")
    img = _buffer(ENTRY[kind][0], K, *((Cout, Cin) if transposed else (Cin, Cout)))
    call(entry or ENTRY[kind][1], ptr(w), K, Cin, Cout, *args, ptr(img), stream())
    torch.cuda.synchronize()
    return img.cpu().numpy()


def _check(got, exp, kind):
    if kind in FP16_KINDS:          # behind the planes: the 64-byte trailer (first word max|W|) and the library's slot scratch
        assert len(got) > len(exp)
        got = got[:len(exp)]
    assert got.shape == exp.shape
    assert np.array_equal(got, exp), f"{kind}: first differing byte at {int(np.flatnonzero(got != exp)[0])}"


@pytest.mark.parametrize("shape", [(1, 32, 4), (3, 64, 130)])
@pytest.mark.parametrize("kind", sorted(ENTRY))
def test_image_matches_oracle(kind, shape):
    args = (0, 0) if kind == "bf16_frag" else ()
    _check(_prepare(kind, _weights(shape), *args), _expected(kind, shape), kind)


@pytest.mark.parametrize("kind", STAGE_KINDS)
def test_stage_image_plain_order_for_channels_off_32(kind):
    shape = (2, 12, 20)
    _check(_prepare(kind, _weights(shape)), _expected(kind, shape), kind)


@pytest.mark.parametrize("flip", [0, 1])
@pytest.mark.parametrize("shape", [(3, 32, 64), (3, 64, 32)])
def test_transposed_images_and_pair(shape, flip):
    from cnrma_amd._lib import call, ptr, stream
    W = _weights(shape)
    K, Cin, Cout = shape
    # stage order: W[flip ? K - 1 - k : k]^T, bf16
    got = _prepare("bf16", W, flip, transposed=True, entry="cnrma_sparse_conv_prepare_weights_bf16_t")
    _check(got, _expected("bf16", shape, True, bool(flip)), "bf16")
    # fragment order, single images: flip must not touch the forward image
    tr = _prepare("bf16_frag", W, 1, flip, transposed=True)
    _check(tr, _expected("bf16_frag", shape, True, bool(flip)), "bf16_frag")
    fwd = _prepare("bf16_frag", W, 0, flip)
    _check(fwd, _expected("bf16_frag", shape), "bf16_frag")
    # the pair: both outputs equal the two single-image calls
    w = torch.tensor(W, device="cuda")
    pf = _buffer(ENTRY["bf16_frag"][0], K, Cin, Cout)
    pt = _buffer(ENTRY["bf16_frag"][0], K, Cout, Cin)
    call("cnrma_sparse_conv_prepare_weights_bf16_frag_pair", ptr(w), K, Cin, Cout, flip, ptr(pf), ptr(pt), stream())
    torch.cuda.synchronize()
    assert np.array_equal(pf.cpu().numpy(), fwd) and np.array_equal(pt.cpu().numpy(), tr)


def test_grid_stride_step_runs_at_27x256x256():
    from cnrma_amd._lib import call, ptr, stream
    shape = (27, 256, 256)
    W = _weights(shape)
    assert W.size > 4096 * 256 and 2 * W.size > 8192 * 256              # beyond the block caps: every thread takes a second element
    _check(_prepare("bf16", W), _expected("bf16", shape), "bf16")
    _check(_prepare("f32_frag", W), _expected("f32_frag", shape), "f32_frag")
    w = torch.tensor(W, device="cuda")
    pf, pt = _buffer(ENTRY["bf16_frag"][0], *shape), _buffer(ENTRY["bf16_frag"][0], *shape)
    call("cnrma_sparse_conv_prepare_weights_bf16_frag_pair", ptr(w), *shape, 1, ptr(pf), ptr(pt), stream())
    torch.cuda.synchronize()
    _check(pf.cpu().numpy(), _expected("bf16_frag", shape), "bf16_frag")
    _check(pt.cpu().numpy(), _expected("bf16_frag", shape, True, True), "bf16_frag")


@pytest.mark.parametrize("kind", FP16_KINDS)
def test_fp16_image_of_all_zero_weights_has_scale_one_and_trailer_zero(kind):
    W = np.zeros((1, 32, 4), dtype=np.float32)
    exp = SO.weight_image(kind, W)
    assert not exp.any() and SO.f16_scale(0.0) == 1.0
    _check(_prepare(kind, W), exp, kind)


@pytest.mark.parametrize("kind", FP16_KINDS)
def test_fp16_trailer_is_exactly_max_abs(kind):
    shape = (3, 64, 130)
    W = _weights(shape)
    got = _prepare(kind, W)
    n = 2 * 2 * shape[0] * shape[1] * SO.cout_padded(shape[2])
    assert got[n:n + 4].view(np.float32)[0] == np.abs(W).max()


def test_rejections():
    """argument checks of the entry points: on the host, before any launch"""
    from cnrma_amd._lib import CnrmaError
    for kind in ("f16_frag", "f32_frag", "bf16_frag"):                 # fragment orders need Cin % 32 == 0
        with pytest.raises(CnrmaError):
            _prepare(kind, _weights((2, 12, 20)), *((0, 0) if kind == "bf16_frag" else ()))
    W = _weights((3, 64, 130))
    with pytest.raises(CnrmaError):                                     # the transposed stage image needs Cout % 32 == 0
        _prepare("bf16", W, 0, transposed=True, entry="cnrma_sparse_conv_prepare_weights_bf16_t")
    from cnrma_amd._lib import call, ptr, stream
    w = torch.tensor(W, device="cuda")
    pf, pt = _buffer(ENTRY["bf16_frag"][0], 3, 64, 130), _buffer(ENTRY["bf16_frag"][0], 3, 130, 64)
    with pytest.raises(CnrmaError):                                     # ... and so does the pair
        call("cnrma_sparse_conv_prepare_weights_bf16_frag_pair", ptr(w), 3, 64, 130, 1, ptr(pf), ptr(pt), stream())
