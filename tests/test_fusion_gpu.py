"""GPU tests of the TSDF fusion (cnrma_amd.fusion / csrc/fusion.hip).  The pinned behaviour is the reference's TSDFFusion on the CPU:
the two fixtures recorded from it (tests/golden/make_golden_fusion.py) and, where no fixture exists, tests/fusion_oracle.py, which
the generator asserted to equal the reference bit for bit.  Every comparison is torch.equal -- float volumes are compared as their
bit patterns, so that -0.0 / +0.0 and NaN payloads count as well -- with no tolerance and no excluded voxel."""
import math

import numpy as np
import pytest
import torch

import fusion_oracle as FO
from test_fusion_cpu import load_fixture, oracle_of_fixture

pytestmark = pytest.mark.gpu
CANARY_F, CANARY_I, PAD = -12345.5, -77, 96


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def state_of(f):
    return dict(tsdf=f.tsdf_vol.cpu(), weight=f.weight_vol.cpu(), color=None if f.color_vol is None else f.color_vol.cpu(),
                label=None if f.label_vol is None else f.label_vol.cpu().long())


def assert_state(got, exp):
    """got / exp: dicts of tsdf [N], weight [N], color [3,N] or None, label [N] int64 or None"""
    assert torch.equal(bits(got["tsdf"]), bits(exp["tsdf"])), int((bits(got["tsdf"]) != bits(exp["tsdf"])).sum())
    assert torch.equal(bits(got["weight"]), bits(exp["weight"]))
    assert (got["color"] is None) == (exp["color"] is None) and (got["label"] is None) == (exp["label"] is None)
    if exp["color"] is not None:
        assert torch.equal(bits(got["color"]), bits(exp["color"]))
    if exp["label"] is not None:
        assert torch.equal(got["label"], exp["label"])


def fixture_state(fx):
    return dict(tsdf=torch.from_numpy(fx["tsdf_vol"]), weight=torch.from_numpy(fx["weight_vol"]),
                color=torch.from_numpy(fx["color_vol"]), label=torch.from_numpy(fx["label_vol"]) if "label_vol" in fx else None)


def fixture_inputs(fx):
    return (torch.from_numpy(fx["proj"]), torch.from_numpy(fx["depth"]), torch.from_numpy(fx["color"]),
            torch.from_numpy(fx["label"]) if "label" in fx else None)


def fusion_of_fixture(fx, device):
    from cnrma_amd.fusion import TSDFFusion
    return TSDFFusion(fx["dims"], fx["voxel_size"], fx["origin"], trunc_ratio=fx["trunc_ratio"].item(), device=device, color=True,
                      label="label" in fx)


def look_at(eye, target, focal, cx, cy, up=(0.0, 0.0, 1.0)):
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    f = (target - eye) / np.linalg.norm(target - eye)
    r = np.cross(f, up)
    r /= np.linalg.norm(r)
    R = np.stack((r, np.cross(f, r), f))
    K = np.array([[focal, 0, cx], [0, focal, cy], [0, 0, 1.0]])
    return K @ np.concatenate((R, (-R @ eye)[:, None]), axis=1), R


def ring_scene(dims, V, H, W, seed, vs=0.04, origin=(-0.13, 0.21, 0.4)):
    """V cameras on a ring around the volume, which fills most of each image; depths scattered through the volume's range, with
    zero, negative, NaN and +inf pixels; random colour and labels.  -> dict of CPU tensors"""
    rng = np.random.default_rng(seed)
    ext = vs * np.asarray(dims, np.float64)
    centre, size = np.asarray(origin) + 0.5 * ext, float(np.linalg.norm(ext)) + vs
    dist = 1.0 + size
    proj = np.stack([look_at(centre + [dist * np.cos(a), dist * np.sin(a), 0.3 * dist], centre, 0.8 * W * dist / size, W / 2, H / 2)[0]
                     for a in 2 * np.pi * (np.arange(V) * 0.37 + 0.1)]).astype(np.float32).reshape(V, 3, 4)
    reach = math.hypot(dist, 0.3 * dist)
    depth = rng.uniform(reach - 0.6 * size, reach + 0.6 * size, (V, H, W)).astype(np.float32)
    bad = rng.random((V, H, W))
    depth[bad < 0.03] = np.nan
    depth[(bad > 0.03) & (bad < 0.06)] = 0.0
    depth[(bad > 0.06) & (bad < 0.09)] = np.inf
    depth[(bad > 0.09) & (bad < 0.12)] = -1.0
    return dict(dims=tuple(dims), vs=vs, origin=tuple(origin), proj=torch.from_numpy(proj), depth=torch.from_numpy(depth),
                color=torch.from_numpy(rng.uniform(0, 255, (V, 3, H, W)).astype(np.float32)),
                label=torch.from_numpy(rng.integers(0, 50, (V, H, W)).astype(np.int32)))


def oracle_of_scene(sc, color=True, label=True, **kw):
    return FO.fuse(sc["dims"], sc["vs"], sc["origin"], sc["proj"], sc["depth"], sc["color"] if color else None,
                   sc["label"] if label else None, **kw)


def fusion_of_scene(sc, device, color=True, label=True):
    from cnrma_amd.fusion import TSDFFusion
    return TSDFFusion(sc["dims"], sc["vs"], sc["origin"], device=device, color=color, label=label)


def raw_fuse(sc, device, color=True, label=True, color_vol=True, label_vol=True):
    """cnrma_tsdf_fuse_f32 through the C ABI on volumes that lie inside larger, canary-filled buffers -> (state, buffers)"""
    from cnrma_amd._lib import call, ptr, stream
    X, Y, Z = sc["dims"]
    n = X * Y * Z
    V, H, W = sc["depth"].shape
    buf = dict(tsdf=torch.full((n + 2 * PAD,), CANARY_F, device=device), weight=torch.full((n + 2 * PAD,), CANARY_F, device=device),
               color=torch.full((3 * n + 2 * PAD,), CANARY_F, device=device),
               label=torch.full((n + 2 * PAD,), CANARY_I, dtype=torch.int32, device=device))
    vol = {k: b[PAD:b.numel() - PAD] for k, b in buf.items()}
    vol["tsdf"].fill_(1)
    vol["weight"].fill_(0)
    vol["color"].fill_(0)
    vol["label"].fill_(-1)
    org = torch.tensor(sc["origin"], dtype=torch.float32, device=device)
    ins = {k: sc[k].to(device).contiguous() for k in ("proj", "depth", "color", "label")}
    call("cnrma_tsdf_fuse_f32", ptr(ins["proj"]), ptr(ins["depth"]), ptr(ins["color"]) if color else None,
         ptr(ins["label"]) if label else None, ptr(org), V, H, W, X, Y, Z, sc["vs"], sc["vs"] * 3, math.inf, ptr(vol["tsdf"]),
         ptr(vol["weight"]), ptr(vol["color"]) if color_vol else None, ptr(vol["label"]) if label_vol else None, stream())
    torch.cuda.synchronize()
    for k, b in buf.items():
        canary = CANARY_I if k == "label" else CANARY_F
        assert bool((b[:PAD] == canary).all()) and bool((b[-PAD:] == canary).all()), f"{k}: a canary beside the volume was overwritten"
    return dict(tsdf=vol["tsdf"].cpu(), weight=vol["weight"].cpu(), color=vol["color"].view(3, n).cpu(), label=vol["label"].cpu().long())


# ---------------------------------------------------------------------------------------------------- fixtures
@pytest.mark.parametrize("name", ["general", "edges"])
def test_fixture_one_batched_launch(device, golden_dir, name):
    fx = load_fixture(golden_dir, name)
    f = fusion_of_fixture(fx, device)
    f.integrate(*fixture_inputs(fx))
    assert_state(state_of(f), fixture_state(fx))
    out = f.get_tsdf()
    assert out.voxel_size == fx["voxel_size"] and out.tsdf_vol.shape == fx["dims"] and out.tsdf_vol.is_cuda
    assert torch.equal(bits(out.tsdf_vol), bits(torch.from_numpy(fx["out_tsdf"])))
    assert torch.equal(bits(out.attribute_vols["color"]), bits(torch.from_numpy(fx["out_color"])))
    if name == "edges":
        lab = out.attribute_vols["instance"]
        assert lab.dtype == torch.int64 and torch.equal(lab.cpu(), torch.from_numpy(fx["out_label"]))
    else:
        assert sorted(out.attribute_vols) == ["color"]


@pytest.mark.parametrize("name", ["general", "edges"])
def test_fixture_every_prefix_of_views(device, golden_dir, name):
    fx = load_fixture(golden_dir, name)
    states = oracle_of_fixture(fx, history=True)
    P, D, C, L = fixture_inputs(fx)
    f = fusion_of_fixture(fx, device)
    for k in range(1, len(P) + 1):
        f.reset()
        f.integrate(P[:k], D[:k], C[:k], None if L is None else L[:k])
        assert_state(state_of(f), states[k - 1])


# ---------------------------------------------------------------------------------------------------- batching
def test_batched_single_and_chunked_launches_agree(device, golden_dir):
    fx = load_fixture(golden_dir, "general")
    P, D, C, _ = fixture_inputs(fx)
    f = fusion_of_fixture(fx, device)
    for v in range(len(P)):
        f.integrate(P[v], D[v], C[v])                                  # the one-view form: [3,4], [H,W], [3,H,W]
    assert_state(state_of(f), fixture_state(fx))
    f.reset()
    f.integrate(P[:2], D[:2], C[:2])
    f.integrate(P[2:], D[2:], C[2:])
    assert_state(state_of(f), fixture_state(fx))


def test_no_views_is_a_no_op(device):
    sc = ring_scene((3, 5, 7), 2, 8, 12, seed=3)
    f = fusion_of_scene(sc, device)
    f.integrate(sc["proj"], sc["depth"], sc["color"], sc["label"])
    before = state_of(f)
    f.integrate(sc["proj"][:0], sc["depth"][:0], sc["color"][:0], sc["label"][:0])
    assert_state(state_of(f), before)
    assert_state(before, oracle_of_scene(sc))


def test_sixty_five_views_in_one_launch(device):
    sc = ring_scene((3, 5, 7), 65, 8, 12, seed=4)
    f = fusion_of_scene(sc, device)
    f.integrate(sc["proj"], sc["depth"], sc["color"], sc["label"])
    exp = oracle_of_scene(sc)
    assert float(exp["weight"].max()) > 8                              # many views really land on one voxel
    assert_state(state_of(f), exp)


# ---------------------------------------------------------------------------------------------------- volume sizes
@pytest.mark.parametrize("dims", [(1, 1, 1), (3, 5, 7), (2, 2, 63), (2, 2, 64), (2, 2, 65), (1, 257, 1), (3, 171, 1)])
def test_volume_sizes_inside_canaried_buffers(device, dims):
    """one voxel; odd extents; z-runs of one wave less one, exactly, plus one; N = 257 and 513: one above a multiple of the block"""
    sc = ring_scene(dims, 3, 16, 20, seed=sum(dims))
    exp = oracle_of_scene(sc)
    assert dims == (1, 1, 1) or float(exp["weight"].max()) > 0
    assert_state(raw_fuse(sc, device), exp)


def test_rejected_arguments(device):
    from cnrma_amd import _lib
    from cnrma_amd._lib import ptr, stream
    lib = _lib.load()
    proj, depth, org, tsdf, weight = (torch.zeros(64, device=device) for _ in range(5))
    t = torch.zeros(64, device=device)
    i = torch.zeros(64, dtype=torch.int32, device=device)

    def rc(V=1, H=2, W=2, X=2, Y=2, Z=2, color=None, label=None, color_vol=None, label_vol=None):
        return lib.cnrma_tsdf_fuse_f32(ptr(proj), ptr(depth), color, label, ptr(org), V, H, W, X, Y, Z, 0.04, 0.12, math.inf, ptr(tsdf),
                                       ptr(weight), color_vol, label_vol, stream())
    assert rc() == 0 and rc(V=0) == 0 and rc(X=0) == 0
    for bad in (dict(V=-1), dict(H=-1), dict(W=-1), dict(X=-1), dict(Y=-1), dict(Z=-1), dict(X=2048, Y=2048, Z=512),
                dict(H=1 << 24), dict(W=1 << 24), dict(color=ptr(t)), dict(label=ptr(i))):
        assert rc(**bad) == -22, bad
    assert rc(color=ptr(t), color_vol=ptr(torch.zeros(64, device=device)), label=ptr(i), label_vol=ptr(torch.zeros_like(i))) == 0
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------- options
@pytest.mark.parametrize("color,label", [(False, True), (True, False), (False, False)])
def test_options(device, color, label):
    sc = ring_scene((6, 5, 9), 4, 16, 20, seed=11)
    f = fusion_of_scene(sc, device, color, label)
    assert (f.color_vol is not None) == color and (f.label_vol is not None) == label
    f.integrate(sc["proj"], sc["depth"], sc["color"], sc["label"])      # images without a volume are ignored, as in the reference
    assert_state(state_of(f), oracle_of_scene(sc, color, label))
    assert sorted(f.get_tsdf("semseg").attribute_vols) == (["color"] if color else []) + (["semseg"] if label else [])
    # through the C ABI: a volume whose image is NULL keeps its contents
    got = raw_fuse(sc, device, color, label)
    exp = oracle_of_scene(sc, color, label)
    assert torch.equal(bits(got["tsdf"]), bits(exp["tsdf"])) and torch.equal(bits(got["weight"]), bits(exp["weight"]))
    if not color:
        assert bool((got["color"] == 0).all())
    if not label:
        assert bool((got["label"] == -1).all())
    got = raw_fuse(sc, device, False, False, color_vol=False, label_vol=False)
    assert torch.equal(bits(got["tsdf"]), bits(exp["tsdf"])) and bool((got["color"] == 0).all()) and bool((got["label"] == -1).all())


def test_max_depth_equals_masking_beforehand(device):
    sc = ring_scene((6, 5, 9), 4, 16, 20, seed=12)
    finite = sc["depth"][torch.isfinite(sc["depth"])]
    cut = float(finite.median())
    assert cut in finite                                                # depth == max_depth itself is kept (d > max_depth masks)
    f = fusion_of_scene(sc, device)
    f.integrate(sc["proj"], sc["depth"], sc["color"], sc["label"], max_depth=cut)
    masked = sc["depth"].clone()
    masked[masked > cut] = 0                                            # generate_tsdf.py:119
    g = fusion_of_scene(sc, device)
    g.integrate(sc["proj"], masked, sc["color"], sc["label"])
    assert_state(state_of(f), state_of(g))
    exp = FO.fuse(sc["dims"], sc["vs"], sc["origin"], sc["proj"], masked, sc["color"], sc["label"])
    assert_state(state_of(f), exp)
    assert not torch.equal(exp["weight"], oracle_of_scene(sc)["weight"])           # the mask really removes observations


def test_input_layouts(device):
    sc = ring_scene((6, 5, 9), 3, 16, 20, seed=13)
    wide = torch.full((3, 16, 40), 7.0)
    wide[:, :, ::2] = sc["depth"]
    strided = wide[:, :, ::2]
    assert not strided.is_contiguous()
    f = fusion_of_scene(sc, device)
    f.integrate(sc["proj"].double().numpy(), strided.to(device), sc["color"].to(device), sc["label"].long())
    assert_state(state_of(f), oracle_of_scene(sc))


# ---------------------------------------------------------------------------------------------------- state
def test_reset_and_get_tsdf_between_integrations(device, golden_dir):
    fx = load_fixture(golden_dir, "edges")
    P, D, C, L = fixture_inputs(fx)
    states = oracle_of_fixture(fx, history=True)
    f = fusion_of_fixture(fx, device)
    f.integrate(P[:2], D[:2], C[:2], L[:2])
    first = f.get_tsdf()
    t, c = FO.finish(states[1])
    assert torch.equal(bits(first.tsdf_vol), bits(t.view(fx["dims"]))) and torch.equal(bits(first.attribute_vols["color"]), bits(c.view((3,) + fx["dims"])))
    assert_state(state_of(f), states[1])                                # get_tsdf left the running sums alone
    f.integrate(P[2:], D[2:], C[2:], L[2:])
    second = f.get_tsdf()
    assert torch.equal(bits(second.tsdf_vol), bits(torch.from_numpy(fx["out_tsdf"])))
    assert torch.equal(second.attribute_vols["instance"].cpu(), torch.from_numpy(fx["out_label"]))
    assert torch.equal(bits(first.tsdf_vol), bits(t.view(fx["dims"])))  # and the first result is its own copy
    f.reset()
    assert_state(state_of(f), FO.initial_state(fx["dims"], True, True))
    f.integrate(P, D, C, L)
    assert_state(state_of(f), fixture_state(fx))


# ---------------------------------------------------------------------------------------------------- scale
def test_full_size_volume(device):
    """192x192x80 voxels (flat indices beyond 2^21, 11520 blocks), two views of 120x160"""
    sc = ring_scene((192, 192, 80), 2, 120, 160, seed=21, origin=(-3.1, -2.9, -0.2))
    f = fusion_of_scene(sc, device, label=False)
    f.integrate(sc["proj"], sc["depth"], sc["color"])
    exp = oracle_of_scene(sc, label=False)
    assert int((exp["weight"] > 0).sum()) > 10000 and int((exp["weight"] == 2).sum()) > 100
    assert_state(state_of(f), exp)


# ---------------------------------------------------------------------------------------------------- end to end
SPHERE_R, SPHERE_VS = 0.5, 0.04


def sphere_scene():
    """depth maps of a sphere of radius 0.5 m from six cameras on the axes, 1.6 m from its centre; pixels whose ray misses it
    hold 0.  The volume is 36^3 voxels of 0.04 m around it."""
    dims, H, W, focal = (36, 36, 36), 96, 128, 100.0
    centre = np.array([0.31, -0.27, 0.9])
    origin = tuple(centre - 0.5 * SPHERE_VS * 36 + 0.013)
    v, u = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    rays = np.stack(((u - W / 2) / focal, (v - H / 2) / focal, np.ones_like(u)), axis=-1)
    proj, depth = [], []
    for axis in range(3):
        for sign in (-1.0, 1.0):
            eye = centre.copy()
            eye[axis] += sign * 1.6
            P, R = look_at(eye, centre, focal, W / 2, H / 2, up=(1.0, 0.0, 0.0) if axis == 2 else (0.0, 0.0, 1.0))
            d = rays @ R                                                # world directions with unit camera-z: t is the depth
            oc = eye - centre
            a, b, c = (d * d).sum(-1), 2 * (d @ oc), oc @ oc - SPHERE_R ** 2
            disc = b * b - 4 * a * c
            t = (-b - np.sqrt(np.maximum(disc, 0))) / (2 * a)
            proj.append(P)
            depth.append(np.where(disc > 0, t, 0.0))
    return dict(dims=dims, vs=SPHERE_VS, origin=origin, centre=centre, proj=torch.from_numpy(np.stack(proj).astype(np.float32)),
                depth=torch.from_numpy(np.stack(depth).astype(np.float32)), color=None, label=None)


def sphere_vertex_error(vertices, centre):
    return np.abs(np.linalg.norm(np.asarray(vertices, np.float64) - centre, axis=1) - SPHERE_R)


def test_sphere_end_to_end(device):
    """fused volume == oracle; the device mesh of it is not empty and every vertex lies within 2 trunc_margin of the sphere: a sign
    change needs a view with |pz - d| < trunc_margin at one end of the edge, plus one voxel and the half-pixel shift of the ray.
    (On the CPU, oracle volume + tests/mesh_oracle.py: 4794 vertices, largest distance 0.1346 m = 1.12 trunc_margin.)"""
    sc = sphere_scene()
    exp = oracle_of_scene(sc, False, False)
    f = fusion_of_scene(sc, device, False, False)
    f.integrate(sc["proj"], sc["depth"])
    assert_state(state_of(f), exp)
    tsdf = f.get_tsdf()
    assert torch.equal(bits(tsdf.tsdf_vol), bits(FO.finish(exp)[0].view(sc["dims"])))
    mesh = tsdf.get_mesh_device().cpu()
    assert len(mesh.vertices) > 1000 and len(mesh.faces) > 1000
    err = sphere_vertex_error(mesh.vertices.numpy(), sc["centre"])
    print(f"sphere: {len(mesh.vertices)} vertices, largest distance from the sphere {err.max():.4f} m")
    assert err.max() <= 2 * 3 * SPHERE_VS
