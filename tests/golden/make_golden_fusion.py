"""Generator of the TSDF-fusion fixtures (not collected by pytest; run in the build container, where the reference is mounted):

    python tests/golden/make_golden_fusion.py            # writes tsdf_fusion_general.npz and tsdf_fusion_edges.npz beside this file

It imports the reference's data_prepare/scannet/tsdf.py from where it lies (scikit-image, trimesh and matplotlib stubbed: absent
here and not used by the fusion), runs TSDFFusion(device='cpu') one frame at a time, asserts that tests/fusion_oracle.py equals it
bit for bit after EVERY view and on every saved array, asserts that each named edge case occurs, and saves inputs and results.  No
reference source is copied: only what its class computes is saved.  The archives are written with a fixed time stamp, so running
the generator again reproduces them byte for byte."""
import importlib.util
import io
import os
import sys
import types
import zipfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF_TSDF = os.path.join(os.environ.get("CNRMA_REFERENCE", "/root/reference"), "data_prepare", "scannet", "tsdf.py")
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import fusion_oracle as FO  # noqa: E402


def load_reference():
    for name, attrs in (("skimage", dict(measure=None)), ("trimesh", {}), ("matplotlib", {}),
                        ("matplotlib.cm", dict(get_cmap=None))):
        if name not in sys.modules:
            m = types.ModuleType(name)
            m.__dict__.update(attrs)
            sys.modules[name] = m
    spec = importlib.util.spec_from_file_location("reference_scannet_tsdf", REF_TSDF)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def save_npz(path, arrays):
    """np.load-compatible compressed archive with a fixed time stamp (np.savez_compressed stamps the current time)"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED, compresslevel=9) as zf:
        for key in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.require(arrays[key], requirements="C"), allow_pickle=False)     # 0-d stays 0-d
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            zf.writestr(info, buf.getvalue(), compresslevel=9)


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def run_case(ref, name, dims, voxel_size, origin, proj, depth, color, label, max_depth=None):
    """the reference frame by frame beside the oracle; -> (arrays to save, oracle states after every view)"""
    fusion = ref.TSDFFusion(dims, voxel_size, origin, trunc_ratio=3, device=torch.device("cpu"), color=color is not None,
                            label=label is not None)
    states = FO.fuse(dims, voxel_size, origin, proj, depth, color, label, trunc_ratio=3, max_depth=max_depth, history=True)
    for v in range(proj.shape[0]):
        d = depth[v].clone()
        if max_depth is not None:
            d[d > max_depth] = 0                                   # generate_tsdf.py:119
        fusion.integrate(proj[v], d, None if color is None else color[v], None if label is None else label[v].long())
        s = states[v]
        assert bits_equal(fusion.tsdf_vol.numpy(), s["tsdf"].numpy()), (name, v, "tsdf")
        assert bits_equal(fusion.weight_vol.numpy(), s["weight"].numpy()), (name, v, "weight")
        if color is not None:
            assert bits_equal(fusion.color_vol.numpy(), s["color"].numpy()), (name, v, "color")
        if label is not None:
            assert bits_equal(fusion.label_vol.numpy(), s["label"].numpy()), (name, v, "label")
    out = fusion.get_tsdf()
    ft, fc = FO.finish(states[-1])
    assert bits_equal(out.tsdf_vol.numpy().reshape(-1), ft.numpy())
    arrays = dict(dims=np.asarray(dims, np.int64), voxel_size=np.float64(voxel_size), origin=np.asarray(origin, np.float64),
                  trunc_ratio=np.int64(3), proj=proj.numpy(), depth=depth.numpy(),
                  tsdf_vol=fusion.tsdf_vol.numpy(), weight_vol=fusion.weight_vol.numpy(), out_tsdf=out.tsdf_vol.numpy())
    if max_depth is not None:
        arrays["max_depth"] = np.float64(max_depth)
    if color is not None:
        assert bits_equal(out.attribute_vols["color"].numpy().reshape(3, -1), fc.numpy())
        arrays.update(color=color.numpy(), color_vol=fusion.color_vol.numpy(), out_color=out.attribute_vols["color"].numpy())
    if label is not None:
        assert bits_equal(out.attribute_vols["instance"].numpy().reshape(-1), states[-1]["label"].numpy())
        arrays.update(label=label.numpy().astype(np.int32), label_vol=fusion.label_vol.numpy(),
                      out_label=out.attribute_vols["instance"].numpy())
    return arrays, states


def look_at(eye, target, focal, cx, cy):
    """3x4 projection K [R | t] of a camera at `eye` looking at `target`, world z up, image y down"""
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    f = (target - eye) / np.linalg.norm(target - eye)
    r = np.cross(f, [0.0, 0.0, 1.0])
    r /= np.linalg.norm(r)
    d = np.cross(f, r)
    R = np.stack((r, d, f))
    K = np.array([[focal, 0, cx], [0, focal, cy], [0, 0, 1.0]])
    return (K @ np.concatenate((R, (-R @ eye)[:, None]), axis=1)).astype(np.float32)


def general_case(ref):
    """40x36x24 voxels of 0.04 m, five views of 48x64 on a ring: noisy depth of 1.2-1.6 m, a near band at 0.3 m, rectangles of
    0, -1, NaN and +inf depth, random colour"""
    dims, vs, origin = (40, 36, 24), 0.04, (-0.81, -0.7, -0.5)
    rng = np.random.default_rng(20240611)
    centre = np.asarray(origin) + 0.5 * vs * np.asarray(dims)
    H, W, V = 48, 64, 5
    proj = np.stack([look_at(centre + [1.5 * np.cos(a), 1.5 * np.sin(a), 0.35], centre, 60.0, 32.0, 24.0)
                     for a in 2 * np.pi * (np.arange(V) + 0.25) / V])
    depth = rng.uniform(1.2, 1.6, (V, H, W)).astype(np.float32)
    depth[:, 4:9, :] = 0.3
    depth[:, 14:20, 6:16] = 0.0
    depth[:, 22:28, 20:30] = -1.0
    depth[:, 30:36, 34:44] = np.nan
    depth[:, 38:44, 48:58] = np.inf
    color = rng.uniform(0.0, 255.0, (V, 3, H, W)).astype(np.float32)
    arrays, states = run_case(ref, "general", dims, vs, origin, torch.from_numpy(proj), torch.from_numpy(depth),
                              torch.from_numpy(color), None)
    w = states[-1]["weight"]
    assert (w > 1).any() and (w == 0).any() and ((w == 0) & (states[-1]["tsdf"] == -1)).any()
    return arrays


def edges_case(ref):
    """16x12x8 voxels of 0.5 at the origin, colour and labels on, four views of 8x12:
    view 0: exact .5 ties in px (pz == 2 everywhere), depth rows cycling 0 / 2.0 / 1.9;
    view 1: pz = wz - 2 below, at and above zero (NaN and inf pixels), depth 0.7;
    view 2: depth 50 everywhere: every voxel it sees gets dist == -1, and those of weight 0 get tsdf == -1 with weight still 0;
    view 3: the same camera with depths around the volume: overwrites some of those voxels, and the labels of view 0's voxels"""
    dims, vs, origin = (16, 12, 8), 0.5, (0.0, 0.0, 0.0)
    H, W = 8, 12
    rng = np.random.default_rng(7)
    proj = np.array([[[2, 0, .5, 1], [0, 2, .25, .5], [0, 0, 0, 2]],
                     [[4, 0, 3, -6], [0, 4, 3, -6], [0, 0, 1, -2]],
                     [[1, 0, 3, 0], [0, 1, 2, 0], [0, 0, 1, .25]],
                     [[1, 0, 3, 0], [0, 1, 2, 0], [0, 0, 1, .25]]], np.float32)
    depth = np.empty((4, H, W), np.float32)
    depth[0] = np.asarray([0.0, 2.0, 1.9], np.float32)[np.arange(H) % 3][:, None]
    depth[1] = 0.7
    depth[2] = 50.0
    depth[3] = rng.uniform(0.5, 3.5, (H, W)).astype(np.float32)
    color = rng.uniform(0.0, 1.0, (4, 3, H, W)).astype(np.float32)
    label = (rng.integers(0, 40, (4, H, W)) + 100 * np.arange(4)[:, None, None]).astype(np.int64)
    P, D = torch.from_numpy(proj), torch.from_numpy(depth)
    arrays, states = run_case(ref, "edges", dims, vs, origin, P, D, torch.from_numpy(color), torch.from_numpy(label))
    # ---- each named case occurs
    world = FO.world_points(dims, vs, origin)
    cam0, cam1 = FO.matmul_fma_chain(P[0], world), FO.matmul_fma_chain(P[1], world)
    q = cam0[0] / cam0[2]
    ties = int(((q - torch.floor(q)) == 0.5).sum())
    pz0 = int((cam1[2] == 0).sum())
    bad_px = cam1[0] / cam1[2]
    assert ties > 0 and pz0 > 0 and torch.isnan(bad_px).any() and torch.isinf(bad_px).any()
    parked = (states[2]["weight"] == 0) & (states[2]["tsdf"] == -1)
    overwritten = parked & (states[3]["tsdf"] != -1)
    assert parked.any() and overwritten.any()
    relabelled = (states[0]["label"] >= 0) & (states[3]["label"] >= 300)
    assert relabelled.any()
    print(f"edges: {ties} ties, {pz0} voxels with pz == 0, {int(parked.sum())} voxels parked at -1 with weight 0, "
          f"{int(overwritten.sum())} of them overwritten, {int(relabelled.sum())} labels overwritten")
    return arrays


if __name__ == "__main__":
    ref = load_reference()
    for name, case in (("tsdf_fusion_general", general_case), ("tsdf_fusion_edges", edges_case)):
        path = os.path.join(HERE, name + ".npz")
        save_npz(path, case(ref))
        size = os.path.getsize(path)
        assert size < 1000000, (name, size)
        print(f"{name}.npz: {size} bytes")
