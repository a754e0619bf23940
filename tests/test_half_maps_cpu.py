"""The C-ABI of the 16-bit feature-map entry points, without a GPU: the symbols exist in the product library and every invalid
call is refused with CNRMA_EINVAL before anything is launched.  All device pointers are NULL except the one under test, so a
call that slipped through the validation would come back with a HIP error code (or, worse, launch): neither is -22."""
import ctypes
import os

import pytest

EINVAL = -22
F16, BF16 = 1, 2
SYMBOLS = ("cnrma_backproject_accum_h16", "cnrma_rma_neus_emit_rows_h16", "cnrma_nchw_to_nhwc_b16", "cnrma_rma_emit_features_h16")


@pytest.fixture(scope="module")
def lib():
    from cnrma_amd import _lib
    if not os.path.exists(_lib.LIB_PATH) or not os.path.exists(_lib.EXP_LIB_PATH):   # fresh checkout: hipcc cross-compiles without a GPU
        import subprocess
        subprocess.run(["make", "-C", os.path.dirname(_lib.LIB_PATH), "-j8"], check=True)
    return _lib.load(experiments=False)


def test_the_symbols_exist_and_the_abi_is_7(lib):
    from cnrma_amd import _lib
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in SYMBOLS:
        assert hasattr(raw, name), name
        assert name in _lib.SIGNATURES
    assert lib.cnrma_abi_version() == 7 == _lib.ABI_VERSION


def _dense(lib, feat, ref, elem, V=3, C=16):
    return lib.cnrma_backproject_accum_h16(feat, ref, elem, None, V, C, 30, 40, 8, 8, 8, 0.04, 0.0, 0.0, 0.0, None, None, None, 0, None)


def _emit(lib, feat, ref, elem, V=3, C=16):
    return lib.cnrma_rma_neus_emit_rows_h16(None, feat, ref, elem, V, C, 30, 40, 300, 0.01, None, 64, None, None, 0, None, 0, None,
                                            None, 0.0, 0.0, 0.0, None, 3, None, 0, None, C, None, None)


ALIGNED, OTHER = 0x1000, 0x2000          # never dereferenced: every call below is refused


@pytest.mark.parametrize("entry", [_dense, _emit], ids=["backproject_accum_h16", "neus_emit_rows_h16"])
def test_invalid_calls_are_refused_before_anything_is_launched(lib, entry):
    for elem in (0, 3):
        assert entry(lib, ALIGNED, None, elem) == EINVAL, elem                  # unknown element code
    for elem in (F16, BF16):
        assert entry(lib, ALIGNED, OTHER, elem) == EINVAL                       # both map pointers
        assert entry(lib, None, None, elem) == EINVAL                           # neither
        assert entry(lib, ALIGNED, None, elem, C=12) == EINVAL                  # C % 8 != 0: no 16-byte load of 8 channels
        assert entry(lib, None, OTHER, elem, C=12) == EINVAL
        assert entry(lib, 0x1002, None, elem) == EINVAL                         # a direct pointer that is not 16-byte aligned
        assert entry(lib, ALIGNED, None, elem, V=0) == EINVAL                   # a bad dimension
        assert entry(lib, None, OTHER, elem, V=0) == EINVAL


def test_point_feature_emission_and_layout_pass_validate_too(lib):
    for elem, feat, ref, C in ((0, ALIGNED, None, 16), (3, ALIGNED, None, 16), (F16, ALIGNED, OTHER, 16), (BF16, None, None, 16),
                               (F16, ALIGNED, None, 12), (BF16, 0x1002, None, 16)):
        assert lib.cnrma_rma_emit_features_h16(feat, ref, elem, C, None, 64, None, None, None, C, None, None) == EINVAL
    assert lib.cnrma_nchw_to_nhwc_b16(None, None, 2, 8, 4, 4, None) == EINVAL
    assert lib.cnrma_nchw_to_nhwc_b16(ALIGNED, OTHER, 0, 8, 4, 4, None) == EINVAL
