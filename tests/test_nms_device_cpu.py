"""The C-ABI surface of the per-class device NMS (no GPU needed): cnrma_nms_classes_workspace_bytes and cnrma_nms_classes_f32 are
declared in include/cnrma.h, exported by both libraries and bound in the ctypes table -- as additions: the ABI version stays 7."""
import ctypes
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"cnrma_nms_classes_workspace_bytes": 2, "cnrma_nms_classes_f32": 18}


def _libs():
    from cnrma_amd import _lib
    if not os.path.exists(_lib.LIB_PATH) or not os.path.exists(_lib.EXP_LIB_PATH):   # fresh checkout: hipcc cross-compiles without a GPU
        subprocess.run(["make", "-C", os.path.dirname(_lib.LIB_PATH), "-j8"], check=True)
    return _lib


def test_the_two_entry_points_are_declared_exported_and_bound():
    _lib = _libs()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cnrma.h")).read(), flags=re.S)
    for name, n_args in NEW.items():
        m = re.search(r"\b(?:int|size_t)\s+" + name + r"\s*\(([^;]*?)\)\s*;", src, flags=re.S)
        assert m is not None, f"{name} is not declared in include/cnrma.h"
        assert len(m.group(1).split(",")) == n_args
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == n_args
        for path in (_lib.LIB_PATH, _lib.EXP_LIB_PATH):
            assert hasattr(ctypes.CDLL(path), name), f"{name} is not exported by {os.path.basename(path)}"
    assert _lib.SIGNATURES["cnrma_nms_classes_workspace_bytes"][0] is ctypes.c_size_t
    assert _lib.SIGNATURES["cnrma_nms_classes_f32"][0] is ctypes.c_int


def test_the_abi_version_is_still_7():
    _lib = _libs()
    assert _lib.ABI_VERSION == 7
    assert ctypes.CDLL(_lib.LIB_PATH).cnrma_abi_version() == 7 and ctypes.CDLL(_lib.EXP_LIB_PATH).cnrma_abi_version() == 7


def test_workspace_size_and_row_limit():
    """host arithmetic only: the masks dominate (n_cls x n_cap x ceil(n_cap / 64) words: 38 MB at 4096 rows x 18 classes), and a
    block the entry point would reject (more than 4096 rows, no class) has no size"""
    lib = _libs().load()
    size = lib.cnrma_nms_classes_workspace_bytes
    masks = 18 * 4096 * 64 * 8
    assert masks <= size(4096, 18) <= masks + 18 * 4096 * 8 + 1024
    assert size(65, 1) >= 65 * 2 * 8 + 2 * 65 * 4 + 8
    assert size(4097, 18) == 0 and size(16, 0) == 0 and size(-1, 3) == 0
    assert size(1, 1) % 16 == 0 and size(4000, 17) % 16 == 0
