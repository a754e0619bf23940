"""GPU tests (-m gpu) of the dense unprojection's z-run lane mapping and its 16-byte stores.

A lane of the product kernel owns runs of 4 consecutive z and writes a run as one 16-byte store when its four voxels are in the
grid at consecutive linear indices that start at a multiple of 4, the grid size is a multiple of 4 and the volume pointer is
16-byte aligned; every other run is stored element by element.  The grids here make each of those conditions fail somewhere:
Z not a multiple of 4 (runs that cross a column end, runs that start unaligned), an odd grid size, grids that are no multiple
of the 16 x 16 x 32 brick, every channel path (1, 2, 4 or 8 lanes per voxel, one and two channel sweeps), a view that sees
nothing, and a volume that is a 4-byte-offset view of a larger buffer.
Bars: volume and count bit-exact against the oracle through both entry points; bit-identical to the round-3 lane mapping
(experiments library) at the north-star and at the ScanNet shape."""
import pytest
import torch

from oracle import rma_oracle as O

pytestmark = pytest.mark.gpu


def _scene(V, C, dims, seed, blind_view=True):
    """small maps (30 x 40, stride 4) around `dims`; blind_view: the middle view looks away from the grid (every voxel behind it)"""
    from cnrma_amd import synth
    sc = synth.make_scene((V, C, 30, 40, tuple(dims), 4), seed=seed)
    feat, proj = sc["features"][:, 0], sc["projection"][:, 0].clone()
    if blind_view:
        proj[V // 2, 2] = torch.tensor([0.0, 0.0, 0.0, -1.0])        # depth -1 for every voxel: the view adds nothing anywhere
    return feat, proj, sc


def _launch(feat_nhwc, proj_scaled, dims, by_ref, offset_floats, device):
    """the C entry points with an output volume that starts `offset_floats` floats into a NaN-filled buffer; returns the volume,
    the count and the buffer's guard words (which must stay NaN)"""
    from cnrma_amd import rma
    from cnrma_amd._lib import call, ptr, stream
    V, H, W, C = feat_nhwc.shape
    X, Y, Z = dims
    G = X * Y * Z
    buf = torch.full((C * G + 8,), float("nan"), dtype=torch.float32, device=device)
    volume = buf[offset_floats:offset_floats + C * G]
    assert volume.data_ptr() == buf.data_ptr() + 4 * offset_floats
    count = torch.full((G,), -7, dtype=torch.int32, device=device)
    st = stream()
    ws = rma._dense_workspace(device, st)
    tail = (ptr(proj_scaled), V, C, H, W, X, Y, Z, 0.04, 0.0, 0.0, 0.0, ptr(volume), ptr(count), ptr(ws), ws.numel() * 4, st)
    if by_ref:
        ref = torch.tensor([feat_nhwc.data_ptr()], dtype=torch.int64, device=device)
        call("cnrma_backproject_accum_ref_f32", ptr(ref), *tail)
    else:
        call("cnrma_backproject_accum_f32", ptr(feat_nhwc), *tail)
    torch.cuda.synchronize()
    guards = torch.cat((buf[:offset_floats], buf[offset_floats + C * G:]))
    return volume.view(C, X, Y, Z).cpu(), count.view(X, Y, Z).cpu(), guards.cpu()


def _check(V, C, dims, seed, device, offsets=(0,)):
    from cnrma_amd import rma
    feat, proj, sc = _scene(V, C, dims, seed)
    vol, cnt = O.backproject_accum(dims, 0.04, (0.0, 0.0, 0.0), proj, feat, 4)
    assert int(cnt.max()) > 1                                        # voxels that several views see exist
    single, _ = O.backproject_accum(dims, 0.04, (0.0, 0.0, 0.0), proj[V // 2:V // 2 + 1], feat[V // 2:V // 2 + 1], 4)
    assert not bool(single.any())                                    # the blind view is blind
    nhwc = rma.to_nhwc(feat.to(device))
    ps = rma.scale_projection(proj, 4).to(device)
    for off in offsets:
        for by_ref in (False, True):
            gv, gc, guards = _launch(nhwc, ps, dims, by_ref, off, device)
            assert torch.isnan(guards).all(), (dims, C, off, by_ref)
            assert torch.equal(gc.long(), cnt), (dims, C, off, by_ref)
            assert torch.equal(gv.view(torch.int32), vol.view(torch.int32)), (dims, C, off, by_ref)


@pytest.mark.parametrize("Z", [5, 6, 7, 8, 33, 36])
def test_z_extents_hit_whole_and_broken_runs(device, Z):
    """Z = 8, 36: every in-grid run is whole; 5, 6, 7, 33: runs cross the column end or start at an unaligned index (the grid
    20 x 18 x Z has a size that is a multiple of 4, so aligned and unaligned runs mix); two bricks along x and y, ragged"""
    _check(4, 32, (20, 18, Z), 10 + Z, device)


def test_grid_size_not_a_multiple_of_4(device):
    """9 x 7 x 5 = 315 and 17 x 19 x 37 = 11951 voxels: the planes of the volume are an odd number of floats apart, so no run may
    leave as a 16-byte store and the whole launch takes the element stores"""
    _check(3, 32, (9, 7, 5), 3, device)
    _check(3, 32, (17, 19, 37), 4, device)
    assert (17 * 19 * 37) % 4 != 0 and (9 * 7 * 5) % 4 != 0


def test_grid_larger_than_one_brick_and_ragged(device):
    """40 x 36 x 44: three bricks along x and y, two along z, the last of each cut (44 = 32 + 12: whole runs in a cut brick)"""
    _check(3, 32, (40, 36, 44), 5, device)


@pytest.mark.parametrize("C", [4, 8, 16, 32, 64])
def test_every_channel_path(device, C):
    """1, 2, 4 and 8 lanes per voxel (C = 4, 8, 16, 32) and two channel sweeps (C = 64), on a grid with whole and broken runs"""
    _check(3, C, (24, 20, 36), 20 + C, device)
    _check(3, C, (10, 12, 7), 40 + C, device)


@pytest.mark.parametrize("C", [16, 32])
def test_volume_at_a_4_byte_offset(device, C):
    """the output is a view 1, 2 or 3 floats into a larger buffer: no 16-byte store may be issued, nothing outside it is written"""
    _check(3, C, (20, 18, 8), 7, device, offsets=(1, 2, 3, 4))


def _old_and_new(shape, device, seed, extra=()):
    from cnrma_amd import rma, synth
    V, C, H, W, dims, stride = shape
    sc = synth.make_scene(shape, seed=seed, device=device, channels_last=True)
    feat = rma.to_nhwc(sc["features"][:, 0])
    assert feat.data_ptr() == sc["features"].data_ptr()
    proj = rma.scale_projection(sc["projection"][:, 0], stride).to(device)
    vol, cnt = rma.backproject_accum(feat, None, dims, 0.04, (0, 0, 0), stride, proj_scaled=proj)       # product library
    assert int(cnt.max()) > 1
    try:
        for kw in (dict(zrun=0),) + tuple(extra):
            rma.dense_tuning(**kw)
            v2, c2 = rma.backproject_accum(feat, None, dims, 0.04, (0, 0, 0), stride, proj_scaled=proj)
            assert torch.equal(c2, cnt), kw
            assert torch.equal(v2, vol), kw
            del v2, c2
    finally:
        rma.dense_tuning()


def test_old_and_new_mapping_agree_at_the_scannet_shape(device):
    """product library (z-runs) against the round-3 mapping of the experiments library; also the z-run kernel of the experiments
    library under each store policy (plain, non-temporal, write-through)"""
    from cnrma_amd import synth
    _old_and_new(synth.SHAPES["S"], device, 1, extra=(dict(zrun=1), dict(zrun=1, nt=1), dict(zrun=1, nt=2), dict(zrun=0, nt=1),
                                                      dict(zrun=1, pipe=2), dict(zrun=1, lpv=4), dict(zrun=1, st=32, lockstep=1)))


def test_old_and_new_mapping_agree_at_the_north_star_shape(device):
    from cnrma_amd import synth
    _old_and_new(synth.SHAPES["NS"], device, 0)
