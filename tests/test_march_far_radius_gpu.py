"""GPU tests (-m gpu) of the uncapped free-space radii and of the chained jumps of the march.

The skip table holds two radii per 4 x 4 x 4 block: the head of the buffer keeps min(R, 16), the `far` region (layout in
include/cnrma.h, cnrma_rma_march_tables_f32) R = min(4 r, 252), r = the largest number of blocks such that every block within
Chebyshev distance r exists, is a whole block inside the grid and holds the block's table value bit for bit.  Both are
compared with that definition, evaluated on the host as sliding-window minima / maxima of the block values (not as the
distance transform the device runs).  The march with skipping on must equal the step-by-step march bit for bit and the oracle,
on TSDFs built around the table's own edges: a 61 x 57 x 49 grid (16 x 15 x 13 blocks, a partial block on every axis, radii of
up to 20 voxels at the centre, i.e. past the former cap of 16) and a 61 x 3 x 49 grid (an axis shorter than one block: no
block is whole, every radius is 0)."""
import numpy as np
import pytest
import torch

from helpers import count_mismatch
from oracle import rma_oracle as O

pytestmark = pytest.mark.gpu

DIMS = (61, 57, 49)
FLAT_DIMS = (61, 3, 49)
VS, ORIGIN, N_STEPS, THR, STRIDE = 0.04, (0.0, 0.0, 0.0), 120, 0.05, 4
V, H, W, C = 3, 30, 40, 4
FAR_MAX, OLD_CAP = 252, 16


def _align(n):
    return (n + 255) & ~255


def _far_offset(nb):
    """offset of the far radii in the skip buffer (include/cnrma.h): behind the capped radii and the block values"""
    return _align(nb) + _align(4 * nb)


def _window(a, r, axis, fn):
    """fn (np.min / np.max) over the window [i - r, i + r] along axis, for the i whose window lies inside the array"""
    return fn(np.lib.stride_tricks.sliding_window_view(a, 2 * r + 1, axis=axis), axis=-1)


def _host_radii(bits, dims):
    """block radii by their definition -> (capped at 16, capped at 252), in voxels"""
    X, Y, Z = dims
    bx, by, bz = -(-X // 4), -(-Y // 4), -(-Z // 4)
    NONE = np.int64(1) << 40
    val = np.full((bx, by, bz), NONE, dtype=np.int64)
    fx, fy, fz = X // 4, Y // 4, Z // 4
    if fx and fy and fz:
        blk = bits[:4 * fx, :4 * fy, :4 * fz].reshape(fx, 4, fy, 4, fz, 4).astype(np.int64)
        first = blk[:, 0:1, :, 0:1, :, 0:1]
        same = (blk == first).all(axis=(1, 3, 5))
        val[:fx, :fy, :fz] = np.where(same, first[:, 0, :, 0, :, 0], NONE)
    radius = np.zeros((bx, by, bz), dtype=np.int64)
    for r in range(1, min(bx, by, bz) // 2 + 1):
        if min(bx, by, bz) < 2 * r + 1:
            break
        lo, hi = val, val
        for axis in range(3):
            lo, hi = _window(lo, r, axis, np.min), _window(hi, r, axis, np.max)
        c = val[r:bx - r, r:by - r, r:bz - r]
        ok = (lo == c) & (hi == c) & (c != NONE)              # the whole cube exists and holds the centre's value
        inner = radius[r:bx - r, r:by - r, r:bz - r]
        inner[ok & (inner == r - 1)] = r                      # radii grow one shell at a time
    return np.minimum(4 * radius, OLD_CAP), np.minimum(4 * radius, FAR_MAX)


def _setup(dims, device):
    from cnrma_amd import rma, synth
    proj = synth.camera_projections(V, dims, VS, img_hw=(H * STRIDE, W * STRIDE))
    feats_cpu = torch.round(torch.randn(V, C, H, W, generator=torch.Generator().manual_seed(61)) * 64) / 64
    pinv = rma.projection_inverse(proj, STRIDE)
    return proj, feats_cpu, rma.to_nhwc(feats_cpu.to(device)), pinv.to(device), pinv


def _variants(dims):
    X, Y, Z = dims
    free = np.full(dims, -1.0, np.float32)
    out = [("free", free)]
    for axis in range(3):
        for r in (3, 4, 5, 6):
            for dd in (-1, 0, 1):
                w = 3 + 4 * r + dd                     # voxel distance 4 r + dd from block 0's last layer
                if w >= dims[axis]:
                    continue
                v = free.copy()
                sl = [slice(None)] * 3
                sl[axis] = w
                v[tuple(sl)] = 1.0
                out.append((f"wall{axis}_{w}", v))
    half = free.copy()
    half[X // 2:] = 1.0                                # the cut runs through a block (X // 2 = 30)
    out.append(("halves", half))
    odd = free.copy()
    odd[X // 2, Y // 2, Z // 2] = 0.5
    odd[0, 0, 0] = 0.5
    out.append(("odd_voxels", odd))
    out.append(("noise", np.random.RandomState(5).uniform(-1.0, 1.0, dims).astype(np.float32)))
    nan = free.copy()
    nan[22, min(30, Y - 1), 20] = np.nan
    out.append(("nan", nan))
    return out


def _march_on_off(rma, m, device):
    prev = (rma.SIGMOID_TABLE, rma.MARCH_SKIP)
    try:
        rma.SIGMOID_TABLE, rma.MARCH_SKIP = True, False
        off = m.march()
        rma.MARCH_SKIP = True
        on = m.march()
    finally:
        rma.SIGMOID_TABLE, rma.MARCH_SKIP = prev
    return off, on


def _check_variant(tag, tsdf_np, dims, device, setup):
    """(a) - (d) of one TSDF; returns the far radii and the blocks the oracle's in-grid samples visit"""
    from cnrma_amd import rma
    from cnrma_amd._lib import call, ptr
    from cnrma_amd.rma import stream
    proj, feats_cpu, feats, pinv, pinv_cpu = setup
    X, Y, Z = dims
    tsdf_cpu = torch.from_numpy(tsdf_np)
    tsdf = tsdf_cpu.to(device)
    m = rma._March(feats, pinv, tsdf, dims, VS, ORIGIN, N_STEPS, THR, "neus", 0)
    (c0, w0, k0, o0), (c1, w1, k1, o1) = _march_on_off(rma, m, device)
    # (c) skipping on == off
    assert int(o0[0]) == 0 and int(o1[0]) == 0, tag
    assert torch.equal(c0, c1) and torch.equal(w0, w1), tag
    live = torch.arange(k0.shape[1], device=device)[None, :] < c0[:, None]
    assert torch.equal(k0[live], k1[live]), tag
    # (a), (b) both radii against the definition
    sig = torch.empty_like(tsdf)
    call("cnrma_rma_sigmoid_table_f32", ptr(tsdf), tsdf.numel(), ptr(sig), stream())
    bits = sig.cpu().numpy().view(np.uint32).reshape(X, Y, Z)
    capped, far = _host_radii(bits, dims)
    nb = capped.size
    buf = m._skip.cpu().numpy()
    got_capped = buf[:nb].reshape(capped.shape).astype(np.int64)
    got_far = buf[_far_offset(nb):_far_offset(nb) + nb].reshape(far.shape).astype(np.int64)
    assert (got_capped == capped).all(), (tag, np.argwhere(got_capped != capped)[:5])
    assert (got_far == far).all(), (tag, np.argwhere(got_far != far)[:5])
    # (d) the rows of the skipping march against the oracle, per view
    visited = np.zeros(far.shape, dtype=bool)
    rows_exp, counts = [], []
    for v in range(V):
        ps = O.scale_projection(proj[v], STRIDE)
        o, d = O.ray_params(ps, H, W, pinv_cpu[v])
        _, vid, valid, _ = O.march_samples(o, d, tsdf_cpu, dims, VS, ORIGIN, N_STEPS)
        b = (vid[:, valid] // 4).numpy()
        visited[b[0], b[1], b[2]] = True
        if tag == "nan":
            continue
        r = O.rma_neus_view(ps, feats_cpu[v], tsdf_cpu, dims, VS, ORIGIN, N_STEPS, THR, o_d=(o, d), reference_quirks=False)
        counts.append(0 if r is None else r.shape[0])
        if r is not None:
            rows_exp.append(r)
    if tag != "nan":
        prev = (rma.SIGMOID_TABLE, rma.MARCH_SKIP)
        try:
            rma.SIGMOID_TABLE, rma.MARCH_SKIP = True, True
            rows, per_view = rma.rma_view_rows(feats, pinv, tsdf, dims, VS, ORIGIN, N_STEPS, THR, single_march=True)
        finally:
            rma.SIGMOID_TABLE, rma.MARCH_SKIP = prev
        exp = (torch.cat(rows_exp) if rows_exp else torch.zeros(0, 4 + C)).numpy()
        rows = rows.cpu().numpy()
        assert list(per_view.cpu().numpy()) == counts, tag
        assert torch.equal(c1.view(V, -1).sum(dim=1).cpu(), per_view.cpu()), tag
        assert rows.shape == exp.shape, tag
        assert count_mismatch(rows[:, :3], exp[:, :3]) == 0 and count_mismatch(rows[:, 4:], exp[:, 4:]) == 0, tag
        np.testing.assert_allclose(rows[:, 3], exp[:, 3], rtol=1e-6, atol=0)      # 1 ulp: the libm tail of the CPU sigmoid
        assert count_mismatch(rows[:, 3], exp[:, 3]) <= max(8, rows.shape[0] // 50), tag
    return far, visited, c1


def test_far_radii_and_chained_jumps_at_their_edges(device):
    """every variant: both radius tables equal their definition, skipping on / off give identical counts, fp64 sums and live
    records, the rows equal the oracle's; over the variants, samples are marched through blocks of radius > 16"""
    setup = _setup(DIMS, device)
    far_visited, radii_seen = 0, set()
    for tag, tsdf_np in _variants(DIMS):
        far, visited, cnt = _check_variant(tag, tsdf_np, DIMS, device, setup)
        assert (far[-1] == 0).all() and (far[:, -1] == 0).all() and (far[:, :, -1] == 0).all(), tag       # partial blocks
        far_visited += int((visited & (far > OLD_CAP)).sum())
        radii_seen |= set(np.unique(far).tolist())
        if tag == "free":
            # only the grid's border limits the radii, and nothing but a ray's last in-grid sample (the step out of free space
            # into the outside, which reads tsdf = +1) can be kept: at most one record per ray, and it lies behind every jump
            bx, by, bz = far.shape
            i, j, k = np.meshgrid(np.arange(bx), np.arange(by), np.arange(bz), indexing="ij")
            edge = np.minimum.reduce([i, j, k, bx - 2 - i, by - 2 - j, bz - 2 - k])       # the last block of an axis is partial
            assert (far == 4 * np.maximum(edge, 0)).all()
            assert int(cnt.max()) <= 1
        if tag == "noise":
            assert (far == 0).all()
    assert far_visited > 0 and max(radii_seen) > OLD_CAP and {0, 4, 8, 12, 16, 20} <= radii_seen


def test_far_radii_on_a_grid_thinner_than_a_block(device):
    """61 x 3 x 49: no block is whole, so every radius is 0 and the march takes no jump; the same checks hold"""
    setup = _setup(FLAT_DIMS, device)
    for tag, tsdf_np in _variants(FLAT_DIMS):
        if tag.startswith("wall") and not tag.endswith(("_15", "_16", "_17")):
            continue                                  # the walls of r = 3 are enough where nothing can jump
        far, _, _ = _check_variant(tag, tsdf_np, FLAT_DIMS, device, setup)
        assert (far == 0).all(), tag


def test_fused_layout_march_with_far_jumps_equals_two_launches(device):
    """the layout + march launch reads the same far radii: with skipping on it equals the two launches bit for bit (wall
    variants; C = 256 so that the launch is the fused one: 3 x 19 x 4 layout blocks >= 8 x 3 x 6 march blocks)"""
    from cnrma_amd import rma
    Cf = 256
    assert -(-H * W // 64) * -(-Cf // 64) * V >= 8 * V * -(-W // 16) * -(-H // 16) and (H * W) % 4 == 0
    proj, _, _, pinv, _ = _setup(DIMS, device)
    f = torch.randn(V, Cf, H, W, generator=torch.Generator().manual_seed(7)).to(device)
    prev = (rma.SIGMOID_TABLE, rma.MARCH_SKIP)
    try:
        rma.SIGMOID_TABLE, rma.MARCH_SKIP = True, True
        for tag, tsdf_np in _variants(DIMS):
            if tag not in ("wall0_23", "wall1_28", "wall2_19"):
                continue
            tsdf = torch.from_numpy(tsdf_np).to(device)
            a = rma._March(torch.empty((V, H, W, Cf), device=device), pinv, tsdf, DIMS, VS, ORIGIN, N_STEPS, THR, "neus", 0)
            a.feat.fill_(float("nan"))
            ca, wa, ka, oa = a.march(layout_from=f)
            b = rma._March(rma.to_nhwc(f), pinv, tsdf, DIMS, VS, ORIGIN, N_STEPS, THR, "neus", 0)
            cb, wb, kb, ob = b.march()
            nb = 16 * 15 * 13
            for lo in (0, _far_offset(nb)):
                assert torch.equal(a._skip[lo:lo + nb], b._skip[lo:lo + nb]) and int(a._skip[lo:lo + nb].max()) > 0, tag
            assert torch.equal(a.feat, b.feat) and torch.equal(a.feat, f.permute(0, 2, 3, 1)), tag
            assert int(oa[0]) == 0 and int(ob[0]) == 0, tag
            assert torch.equal(ca, cb) and torch.equal(wa, wb) and int(ca.sum()) > 100, tag
            live = torch.arange(ka.shape[1], device=device)[None, :] < ca[:, None]
            assert torch.equal(ka[live], kb[live]), tag
    finally:
        rma.SIGMOID_TABLE, rma.MARCH_SKIP = prev
