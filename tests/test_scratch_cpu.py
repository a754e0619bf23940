"""The stream-keyed table rule (_lib.lru_get) on plain Python objects, and the sizes rma hands the dense kernel -- the module
whose table moved onto that rule -- against values written out from the formulas of include/cnrma.h."""
import threading

import pytest

from cnrma_amd import _lib


def test_lru_get_hit_returns_the_object_and_makes_it_the_last_to_go():
    table, made = {}, []

    def make(k):
        def f():
            made.append(k)
            return [k]
        return f

    a = _lib.lru_get(table, "a", make("a"), limit=3)
    b = _lib.lru_get(table, "b", make("b"), limit=3)
    c = _lib.lru_get(table, "c", make("c"), limit=3)
    assert _lib.lru_get(table, "a", make("a"), limit=3) is a and made == ["a", "b", "c"]     # a hit builds nothing
    assert list(table) == ["b", "c", "a"]                                                   # ... and moves to the recent end
    _lib.lru_get(table, "d", make("d"), limit=3)                                            # drops b, the least recently used
    assert list(table) == ["c", "a", "d"] and table["a"] is a and table["c"] is c
    assert _lib.lru_get(table, "b", make("b"), limit=3) is not b and list(table) == ["a", "d", "b"]
    _lib.lru_get(table, "e", make("e"), limit=1)                                            # a smaller limit trims the table
    assert list(table) == ["e"]


def test_lru_get_never_exceeds_its_limit():
    table = {}
    for i in range(200):
        _lib.lru_get(table, (i * 7) % 31, object, limit=5)
        assert len(table) <= 5
    table = {}
    for i in range(40):
        _lib.lru_get(table, i, object)
    assert len(table) == _lib.LRU_STREAMS


def test_lru_get_from_eight_threads():
    table, errors = {}, []

    def work(t):
        try:
            for i in range(2000):
                k = (i * (2 * t + 1) + t) % 20
                v = _lib.lru_get(table, k, lambda k=k: (k, object()), limit=12)
                assert v[0] == k
        except BaseException as e:                                       # noqa: BLE001 -- reported by the main thread
            errors.append(e)

    threads = [threading.Thread(target=work, args=(t,)) for t in range(8)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    assert len(table) <= 12 and all(k == v[0] for k, v in table.items())


# dims (40, 40, 16): 2 x 2 x 1 blocks of 32^3, + 7, x 512 lanes x 8 bytes = 45 056 bytes of view masks per 64 views
@pytest.mark.parametrize("V,masks", [(1, 45056), (65, 90112)])
def test_dense_workspace_sizes(V, masks):
    from cnrma_amd import rma
    dims = (40, 40, 16)
    assert rma.DENSE_WORKSPACE_BYTES == 1024 and rma.DENSE_MASK_MIN_SWEEPS == 3
    assert rma.dense_mask_bytes(dims, V) == masks
    # channel sweeps: fp32 maps 4 channels per lane on 2 / 8 / 4 lanes per voxel, 16-bit maps 8 channels on 1 / 4 / 2 lanes
    assert [rma.dense_sweeps(C) for C in (8, 64, 80)] == [1, 2, 5]
    assert [rma.dense_sweeps(C, h16=True) for C in (8, 64, 80)] == [1, 2, 5]
    for h16 in (False, True):
        assert [rma.dense_workspace_bytes(dims, V, C, h16) for C in (8, 64, 80)] == [1024, 1024, 1024 + masks]
    assert rma.dense_workspace_bytes(dims, V) == 1024 + masks                                # C unknown: always room for the masks
