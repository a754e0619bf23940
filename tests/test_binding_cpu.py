"""The ctypes binding is read from include/cnrma.h at import (cnrma_amd._lib._read_header; no GPU needed): the reader against
signatures written out by hand, against synthetic header text, the constants against their #defines, and the bound names against
the two built libraries."""
import ctypes
import os
import subprocess

import pytest

from cnrma_amd import _lib

P, I, L, F, D, Z, U = (ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float, ctypes.c_double, ctypes.c_size_t,
                       ctypes.c_uint32)
# typed here from the C text of the header, parameter by parameter; between them: every scalar type, both return types,
# (void), a `const float* const*`, a prototype of the experiments block
PINNED = {
    "cnrma_abi_version": (I, []),
    "cnrma_sample_mask": (I, [P, L, I, U, P, P, P, P]),
    "cnrma_cloud_voxel_downsample_f32": (I, [P, L, P, D, P, Z, P, P, L, P, P]),
    "cnrma_backproject_accum_ref_f32": (I, [P, P, I, I, I, I, I, I, I, F, F, F, F, P, P, P, L, P]),
    "cnrma_sparse_conv_plan": (I, [L, I, I, I, I, I, Z, P]),
    "cnrma_tsdf_resample_attr_i64": (I, [P, I, I, I, I, P, F, P, P, I, I, I, L, I, P, P]),
    "cnrma_scan_workspace_bytes": (Z, [L]),
    "cnrma_sample_workspace_bytes": (Z, []),
    "cnrma_debug_conv_tuning": (I, [P, I]),
}


@pytest.mark.parametrize("name", PINNED)
def test_pinned_signatures(name):
    table = _lib.EXPERIMENT_SIGNATURES if name.startswith("cnrma_debug_") else _lib.SIGNATURES
    restype, argtypes = table[name]
    want_res, want_args = PINNED[name]
    assert restype is want_res
    assert len(argtypes) == len(want_args) and all(a is b for a, b in zip(argtypes, want_args)), argtypes
    assert name not in (_lib.SIGNATURES if table is _lib.EXPERIMENT_SIGNATURES else _lib.EXPERIMENT_SIGNATURES)


def test_the_tables_keep_their_shape():
    """name -> (restype, [argtypes]), 128 product prototypes and 3 of the experiments library, in header order"""
    assert len(_lib.SIGNATURES) == 128 and len(_lib.EXPERIMENT_SIGNATURES) == 3
    for table in (_lib.SIGNATURES, _lib.EXPERIMENT_SIGNATURES):
        for name, (restype, argtypes) in table.items():
            assert restype in (I, Z) and isinstance(argtypes, list) and all(a in (P, I, L, F, D, Z, U) for a in argtypes), name
    assert next(iter(_lib.SIGNATURES)) == "cnrma_abi_version"


SYNTHETIC = """
/* a comment that quotes one:  int cnrma_quoted(int a);  */
// and another: int cnrma_slashed(void);
#ifndef GUARD
#define GUARD
#define CNRMA_NEG (-22)
#define CNRMA_SEVEN 7   /* int cnrma_in_define_comment(void); */
#define CNRMA_BYTES(X, Y) \\
  (((X) + 31) / 32 * (Y))
#define CNRMA_NOT_AN_INT 1.5
int cnrma_three_lines(const float* a,
                      int64_t  n   /* rows */,
                      const double scale);
size_t cnrma_nothing();
#ifdef CNRMA_EXPERIMENTS
int cnrma_debug_x(const float* const* ref, uint32_t seed);
#endif
int cnrma_after(float const x, size_t n);
#endif
"""


def test_synthetic_header():
    protos, exp, constants = _lib._read_header(SYNTHETIC)
    assert protos == {"cnrma_three_lines": (I, [P, L, D]), "cnrma_nothing": (Z, []), "cnrma_after": (I, [F, Z])}
    assert list(protos) == ["cnrma_three_lines", "cnrma_nothing", "cnrma_after"]            # header order
    assert exp == {"cnrma_debug_x": (I, [P, U])}
    assert constants == {"CNRMA_NEG": -22, "CNRMA_SEVEN": 7}           # no function-like macro, no guard, nothing but integers


@pytest.mark.parametrize("text,words", [
    ("int cnrma_f(const float* a, unsigned n);", ("cnrma_f", "unsigned n")),                 # a scalar the map does not hold
    ("int cnrma_f(const float* a, long long n);", ("cnrma_f", "long long n")),
    ("int cnrma_f(const float* a, uint8_t flag);", ("cnrma_f", "uint8_t flag")),
    ("int cnrma_f(int);", ("cnrma_f", "'int'")),                                             # no name: nothing left to be the type
    ("double cnrma_f(int a);", ("cnrma_f", "double")),                                       # a return type that is neither
    ("int cnrma_f(int a);\nint cnrma_g(void);\nint cnrma_f(int a);", ("cnrma_f", "twice")),
    ("int cnrma_f(int a);\n#ifdef CNRMA_EXPERIMENTS\nint cnrma_f(int a);\n#endif", ("cnrma_f", "twice")),
    ("#ifdef CNRMA_EXPERIMENTS\n#ifdef __cplusplus\nint cnrma_debug_f(int a);\n#endif\n#endif", ("nested", "__cplusplus")),
    ("#ifdef CNRMA_EXPERIMENTS\nint cnrma_debug_f(int a);\n#else\nint cnrma_g(void);\n#endif", ("nested", "#else")),
])
def test_what_the_reader_does_not_know_raises(text, words):
    with pytest.raises(_lib.CnrmaError) as e:
        _lib._read_header(text)
    assert all(w in str(e.value) for w in words), str(e.value)


def test_constants_are_the_headers():
    import torch
    from cnrma_amd import cloud, rma
    c = _lib.CONSTANTS
    assert c["CNRMA_ABI_VERSION"] == 7 == _lib.ABI_VERSION and c["CNRMA_EINVAL"] == -22 == _lib.EINVAL
    assert rma.DENSE_WORKSPACE_BYTES == c["CNRMA_DENSE_WORKSPACE_BYTES"] == 1024
    assert rma.ELEM_CODES == {torch.float16: c["CNRMA_ELEM_F16"], torch.bfloat16: c["CNRMA_ELEM_BF16"]} == {torch.float16: 1, torch.bfloat16: 2}
    assert (cloud.NONFINITE, cloud.VOXEL_TOO_SMALL) == (c["CNRMA_CLOUD_NONFINITE"], c["CNRMA_CLOUD_VOXEL_TOO_SMALL"]) == (1, 2)
    assert "CNRMA_DENSE_MASK_BYTES" not in c and "CNRMA_H" not in c
    assert all(type(v) is int for v in c.values())


def test_the_header_is_found_beside_the_real_package_and_missed_loudly(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert os.path.samefile(_lib.HEADER_PATH, os.path.join(root, "include", "cnrma.h"))
    assert os.path.samefile(os.path.dirname(_lib.__file__), os.path.join(root, "cn-rma_amd"))
    # the module's top level run again on a copy without a header beside it: CnrmaError with the path, no fallback table
    pkg = tmp_path / "pkg"
    pkg.mkdir()
    copy = pkg / "_lib.py"
    copy.write_text(open(_lib.__file__).read())
    with pytest.raises(Exception) as e:
        exec(compile(copy.read_text(), str(copy), "exec"), {"__name__": "_lib_copy", "__file__": str(copy)})
    assert type(e.value).__name__ == "CnrmaError" and str(tmp_path / "include" / "cnrma.h") in str(e.value)


def test_every_bound_name_resolves_in_its_library():
    if not os.path.exists(_lib.LIB_PATH) or not os.path.exists(_lib.EXP_LIB_PATH):   # fresh checkout: hipcc cross-compiles without a GPU
        subprocess.run(["make", "-C", os.path.dirname(_lib.LIB_PATH), "-j8"], check=True)
    product, exp = ctypes.CDLL(_lib.LIB_PATH), ctypes.CDLL(_lib.EXP_LIB_PATH)
    for name in _lib.SIGNATURES:
        assert hasattr(product, name) and hasattr(exp, name), name
    for name in _lib.EXPERIMENT_SIGNATURES:
        assert hasattr(exp, name) and not hasattr(product, name), name
