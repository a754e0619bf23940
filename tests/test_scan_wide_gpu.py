"""GPU tests (-m gpu) of the tiled scans (csrc/util.hip run_scan: cnrma_exclusive_scan_i32, cnrma_mask_to_index) around their
own edges: full tiles take 16-byte accesses on a lane-interleaved item map, the last partial tile and misaligned buffers the
guarded scalar ones; up to TILE tiles the scan is two launches, beyond it three.  Reference: torch.cumsum in int64.

The tile size is read off the library (cnrma_scan_workspace_bytes holds one int per tile + 2); the launch threshold mirrors
run_scan (n_tiles <= TILE: two launches).  Inputs of at most 32 768 items take the one-block kernel, so the tile edges are also
tested at 9 tiles, the first multiple above it."""
import pytest
import torch

pytestmark = pytest.mark.gpu

SINGLE_MAX = 32768


def _tile():
    from cnrma_amd import _lib
    n = 1 << 30
    tiles = (_lib.load().cnrma_scan_workspace_bytes(n) - 64) // 4 - 2
    assert tiles > 0 and n % tiles == 0
    return n // tiles


def _sizes():
    T = _tile()
    return T, [SINGLE_MAX + 1, T - 1, T, T + 1, 3 * T + 5, 9 * T - 1, 9 * T, 9 * T + 1, 11 * T + 5, T * T - 1, T * T, T * T + 1]


def _scan(count, out=None):
    from cnrma_amd import _lib
    from cnrma_amd._lib import call, ptr
    from cnrma_amd.rma import stream
    n = count.numel()
    if out is None:
        out = torch.empty(n + 1, dtype=torch.int32, device=count.device)
    ws = torch.empty(_lib.load().cnrma_scan_workspace_bytes(n), dtype=torch.uint8, device=count.device)
    call("cnrma_exclusive_scan_i32", ptr(count), ptr(out), n, ptr(ws), stream())
    return out


def _index(mask, sel=None):
    from cnrma_amd import _lib
    from cnrma_amd._lib import call, ptr
    from cnrma_amd.rma import stream
    n = mask.numel()
    if sel is None:
        sel = torch.empty(n, dtype=torch.int32, device=mask.device)
    n_sel = torch.full((1,), -7, dtype=torch.int32, device=mask.device)
    ws = torch.empty(_lib.load().cnrma_scan_workspace_bytes(n), dtype=torch.uint8, device=mask.device)
    call("cnrma_mask_to_index", ptr(mask), ptr(sel), ptr(n_sel), n, ptr(ws), stream())
    return sel, n_sel


def _check_scan(count, out):
    n = count.numel()
    inc = torch.cumsum(count, 0, dtype=torch.int64)
    assert int(out[0]) == 0 and torch.equal(out[1:].long(), inc), n


def _check_index(mask, sel, n_sel):
    inc = torch.cumsum(mask, 0, dtype=torch.int64)
    exp = torch.where(mask != 0, inc - 1, torch.full_like(inc, -1))
    assert torch.equal(sel.long(), exp) and int(n_sel) == int(inc[-1]), mask.numel()


def test_tile_size_is_a_power_of_two_above_the_single_block_kernel():
    # (no GPU needed beyond loading the library, but it lives with the tests that depend on it)
    T = _tile()
    assert T & (T - 1) == 0 and 9 * T > SINGLE_MAX and T * T > 12_288_000       # the north-star's 12.3 M rays: two launches


def test_scans_at_tile_and_launch_thresholds(device):
    T, sizes = _sizes()
    g = torch.Generator(device=device).manual_seed(3)
    big = torch.randint(0, 5, (T * T + 1,), generator=g, dtype=torch.int32, device=device)
    for n in sizes:
        count = big[:n]
        _check_scan(count, _scan(count))
        mask = (count > 2).to(torch.uint8)
        _check_index(mask, *_index(mask))


@pytest.mark.parametrize("in_off,out_off", [(1, 0), (0, 1), (1, 1), (2, 3), (4, 0)])
def test_scans_with_misaligned_buffers(device, in_off, out_off):
    """input / output start in_off / out_off ITEMS behind a 16-byte boundary: 4 bytes off for the int32 scan (offset 1), 1, 2
    and 4 bytes off for the byte mask (4 is aligned for its 4-byte loads) -- the wide path must not be taken where it cannot"""
    T = _tile()
    n = 9 * T + 5
    g = torch.Generator(device=device).manual_seed(in_off * 8 + out_off)
    base = torch.randint(0, 7, (n + 8,), generator=g, dtype=torch.int32, device=device)
    count = base[in_off:in_off + n]
    assert count.data_ptr() % 16 == (4 * in_off) % 16
    out = torch.full((n + 1 + 8,), -1, dtype=torch.int32, device=device)
    o = out[out_off:out_off + n + 1]
    _scan(count, o)
    _check_scan(count, o)
    assert (out[:out_off] == -1).all() and (out[out_off + n + 1:] == -1).all()
    mbase = (base > 3).to(torch.uint8)
    mask = mbase[in_off:in_off + n]
    assert mask.data_ptr() % 16 == in_off
    sel_buf = torch.full((n + 8,), -9, dtype=torch.int32, device=device)
    sel = sel_buf[out_off:out_off + n]
    _, n_sel = _index(mask, sel)
    _check_index(mask, sel, n_sel)
    assert (sel_buf[:out_off] == -9).all() and (sel_buf[out_off + n:] == -9).all()


@pytest.mark.parametrize("value", [0, 1])
def test_all_zero_and_all_one_masks(device, value):
    T = _tile()
    for n in (9 * T, 9 * T + 1, 11 * T + 5):
        mask = torch.full((n,), value, dtype=torch.uint8, device=device)
        sel, n_sel = _index(mask)
        _check_index(mask, sel, n_sel)
        assert int(n_sel) == value * n
        _check_scan(mask.int(), _scan(mask.int()))


def test_total_just_under_two_to_the_31(device):
    T = _tile()
    n = 9 * T + 3
    each = (2 ** 31 - 1) // n
    count = torch.full((n,), each, dtype=torch.int32, device=device)
    count[-1] += (2 ** 31 - 1) - each * n
    out = _scan(count)
    _check_scan(count, out)
    assert int(out[-1]) == 2 ** 31 - 1
