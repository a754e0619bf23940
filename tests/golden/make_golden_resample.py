"""Generator of the TSDF-resampling fixtures (not collected by pytest; run in the build container, where the reference is mounted):

    python tests/golden/make_golden_resample.py            # writes tsdf_resample_{general,ties,oblique,attrs}.npz beside this file

It imports the reference's data_prepare/scannet/tsdf.py from where it lies (the TSDF class WITH attribute volumes; scikit-image,
trimesh and matplotlib stubbed: absent here and not used by transform), runs on the CPU, side by side, the reference's
TSDF.transform, the project's TSDF.transform (volume) and tests/resample_oracle.py, asserts that all three are equal bit for bit,
asserts that each named case occurs, and saves inputs and results.  No reference source is copied: only what its class computes is
saved.  The archives are written with a fixed time stamp, so running the generator again reproduces them byte for byte.

The host's matrix product comes from a BLAS, whose summation order is its own; the fixtures pin what it gave HERE (an un-fused sum
from the left, which is what the oracle and the kernel state).  If this generator's assertions ever fail on another machine, that
machine's BLAS sums differently: the fixtures, not its results, are the pin."""
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

import resample_oracle as RO  # noqa: E402
from projects.mvsdetection.datasets.tsdf import TSDF  # noqa: E402


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


def rotation(axis, angle):
    """Rodrigues: rotation by `angle` about `axis`, float64 3x3"""
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def centred(R, src_dim, src_origin, dst_dim, dst_origin, vs, shift=(0.0, 0.0, 0.0)):
    """4x4 float32 (new world -> old world) that rotates by R and maps the centre of the new volume onto the centre of the old
    one, moved by `shift`"""
    sc = np.asarray(src_origin) + 0.5 * vs * np.asarray(src_dim) + np.asarray(shift)
    dc = np.asarray(dst_origin) + 0.5 * vs * np.asarray(dst_dim)
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = sc - R @ dc
    return torch.from_numpy(T.astype(np.float32))


def run_case(ref, name, src, attrs, vs, src_origin, T, dst_dim, dst_origin):
    """reference, project and oracle side by side on the CPU -> (arrays to save, positions of the oracle)"""
    so = torch.tensor(src_origin, dtype=torch.float32).view(1, 3)
    r = ref.TSDF(vs, so, src.clone(), {k: v.clone() for k, v in attrs.items()}).transform(T, list(dst_dim), list(dst_origin))
    p = TSDF(vs, so, src.clone()).transform(T, list(dst_dim), list(dst_origin))
    pos = RO.positions(tuple(src.shape), so, vs, T, dst_dim, dst_origin)
    o = RO.resample_volume(src, pos)
    assert bits_equal(r.tsdf_vol.numpy(), o.numpy()), (name, "reference vs oracle", int((r.tsdf_vol != o).sum()))
    assert bits_equal(p.tsdf_vol.numpy(), o.numpy()), (name, "project vs oracle", int((p.tsdf_vol != o).sum()))
    arrays = dict(src=src.numpy(), voxel_size=np.float64(vs), src_origin=np.asarray(src_origin, np.float64), transform=T.numpy(),
                  dst_dim=np.asarray(dst_dim, np.int64), dst_origin=np.asarray(dst_origin, np.float64), out=r.tsdf_vol.numpy())
    for key, value in attrs.items():
        got = r.attribute_vols[key]
        exp = RO.resample_float(value, pos) if value.dtype.is_floating_point else \
            RO.resample_int(value, pos, fill=-1 if key == "semseg" else None)
        assert got.dtype == value.dtype and bits_equal(got.numpy(), exp.numpy()), (name, key)
        arrays["attr_" + key] = value.numpy()
        arrays["out_" + key] = got.numpy()
    return arrays, pos


def shares(src, pos):
    near = RO.nearest(src.reshape((1,) + tuple(src.shape)), pos)[0]
    border = pos["border"]
    band = ~border & (near.abs() < 1)
    return float(band.float().mean()), float(border.float().mean())


def general_case(ref):
    """64x50x23 voxels of 0.08 m into 48x40x24 under a rotation about z by 0.7 rad and a translation; values random in
    [-1.3, 1.3] clamped to [-1, 1]"""
    rng = np.random.default_rng(20240923)
    dims, vs, so, nd, do = (64, 50, 23), 0.08, (-1.37, 0.55, -0.21), (48, 40, 24), (0.0, 0.0, 0.0)
    src = torch.from_numpy(rng.uniform(-1.3, 1.3, dims).astype(np.float32)).clamp(-1, 1)
    T = centred(rotation((0, 0, 1), 0.7), dims, so, nd, do, vs, shift=(0.31, -0.12, 0.07))
    arrays, pos = run_case(ref, "general", src, {}, vs, so, T, nd, do)
    band, border = shares(src, pos)
    assert band >= 0.10 and 0.10 <= border <= 0.90, (band, border)
    print(f"general: band share {band:.3f}, border share {border:.3f}")
    return arrays


def no_nearest_index_outside_inside_the_border_test():
    """Can the nearest index fall outside the volume while |n| < 1?  It would need s = dim - 0.5 exactly with dim even (rint then
    gives dim).  n = q - 1 with q = 2 c / (dim - 1) a float below 2, so n + 1 = q again, exactly, and s = (q dim - 1) / 2.  The
    largest q is 2 - 2^-23; q dim = 2 dim - dim 2^-23 lies at least half a spacing below 2 dim (exactly representable when dim is
    a power of two), so it never rounds up to 2 dim, and the subtraction and the halving are exact: s < dim - 0.5.  Checked here
    by brute force over every even dim up to 8192 and the 64 largest q: no such voxel can be built with this arithmetic.  The
    bounds test of the nearest sample is therefore exercised by border voxels only -- the 'attrs' fixture's instance volume, which
    is sampled on the border too (and padded with 0 there by that test), and the zero padding of its colour corners."""
    q = torch.tensor(2.0) - torch.arange(1, 65, dtype=torch.float32) * 2.0 ** -23
    for dim in range(2, 8193, 2):
        d = torch.tensor(float(dim))
        n = q - 1
        assert bool((n.abs() < 1).all())
        s = ((n + 1) * d - 1) / 2
        assert bool((torch.round(s) <= dim - 1).all()), dim
    return True


def ties_case(ref):
    """16x12x8 voxels of 0.5 at the origin into 20x14x10 at (-1,-1,-1) under a pure translation by half a voxel along every axis:
    c = index - 1.5 exactly, and s = c dim / (dim - 1) - 0.5 is an exact .5 tie where 2 c = dim - 1 (s = 7.5, 5.5, 3.5: the middle
    of every axis, where ties-to-even decides between two voxels)"""
    rng = np.random.default_rng(11)
    dims, vs, so, nd, do = (16, 12, 8), 0.5, (0.0, 0.0, 0.0), (20, 14, 10), (-1.0, -1.0, -1.0)
    src = torch.from_numpy(rng.uniform(-1.3, 1.3, dims).astype(np.float32)).clamp(-1, 1)
    T = torch.eye(4)
    T[:3, 3] = 0.25
    arrays, pos = run_case(ref, "ties", src, {}, vs, so, T, nd, do)
    s = pos["s"]
    tie = (s - torch.floor(s)) == 0.5
    ties, inside = int(tie.sum()), int((tie & ~pos["border"].unsqueeze(0)).sum())
    assert ties >= 100 and inside >= 100, (ties, inside)
    outside = ((torch.round(s) < 0) | (torch.round(s) >= torch.tensor(dims).view(3, 1))).any(0) & ~pos["border"]
    assert no_nearest_index_outside_inside_the_border_test() and int(outside.sum()) == 0
    print(f"ties: {ties} exact .5 ties in s, {inside} of them in voxels off the border; no nearest index outside the volume "
          f"with |n| < 1 (none can be built: see no_nearest_index_outside_inside_the_border_test)")
    return arrays


def oblique_case(ref):
    """40x36x30 voxels of 0.04 m into 32x32x24 under a rotation by 0.9 rad about (1, 1, 1): an output z-run crosses source rows
    and planes"""
    rng = np.random.default_rng(5)
    dims, vs, so, nd, do = (40, 36, 30), 0.04, (0.4, -0.3, 0.1), (32, 32, 24), (0.0, 0.0, 0.0)
    src = torch.from_numpy(rng.uniform(-1.3, 1.3, dims).astype(np.float32)).clamp(-1, 1)
    T = centred(rotation((1, 1, 1), 0.9), dims, so, nd, do, vs)
    arrays, pos = run_case(ref, "oblique", src, {}, vs, so, T, nd, do)
    band, border = shares(src, pos)
    r = torch.round(pos["s"]).view(3, 32 * 32, 24)
    crossing = ((r[0].max(1).values != r[0].min(1).values) & (r[1].max(1).values != r[1].min(1).values)).float().mean()
    assert band >= 0.10 and 0.05 <= border <= 0.90 and float(crossing) > 0.9, (band, border, float(crossing))
    print(f"oblique: band share {band:.3f}, border share {border:.3f}, z-runs that change source x and y: {float(crossing):.3f}")
    return arrays


def attrs_case(ref):
    """20x18x12 voxels of 0.08 m into 24x20x16 under a rotation about z and a small tilt, with 'color' [3,X,Y,Z] float32,
    'instance' int64 (no fill: zero padding on the border) and 'semseg' int64 (-1 on the border)"""
    rng = np.random.default_rng(3)
    dims, vs, so, nd, do = (20, 18, 12), 0.08, (-0.2, 0.1, 0.3), (24, 20, 16), (0.0, 0.0, 0.0)
    src = torch.from_numpy(rng.uniform(-1.3, 1.3, dims).astype(np.float32)).clamp(-1, 1)
    attrs = dict(color=torch.from_numpy(rng.uniform(0, 255, (3,) + dims).astype(np.float32)),
                 instance=torch.from_numpy(rng.integers(1, 60, dims)), semseg=torch.from_numpy(rng.integers(1, 41, dims)))
    T = centred(rotation((0.2, -0.1, 1), 0.4), dims, so, nd, do, vs, shift=(0.05, 0.0, -0.04))
    arrays, pos = run_case(ref, "attrs", src, attrs, vs, so, T, nd, do)
    border = pos["border"].view(nd)
    inst, sem, col = (torch.from_numpy(arrays["out_" + k]) for k in ("instance", "semseg", "color"))
    # instance: not filled, so its border voxels are sampled, and the bounds test of the nearest sample makes them 0 (s >= dim - 0.5
    # or s <= -0.5 there: only an exact s == -0.5 would still read voxel 0); semseg: -1 exactly on the border
    assert (inst[border] == 0).any() and (inst[~border] > 0).all()
    assert (sem[border] == -1).all() and (sem[~border] > 0).all()
    # colour: voxels off the border whose upper or lower corners are padding (the bounds test of the corners)
    f = torch.floor(pos["s"])
    d = torch.tensor(dims, dtype=torch.float32).view(3, 1)
    padded = (((f < 0) | (f + 1 >= d)).any(0) & ~pos["border"] & (f + 1 >= 0).all(0) & (f < d).all(0))
    assert int(padded.sum()) >= 100 and (col != 0).any()
    print(f"attrs: border share {float(border.float().mean()):.3f}, {int((inst[border] == 0).sum())} border voxels whose instance "
          f"sample is padding, {int(padded.sum())} voxels off the border with padded colour corners")
    return arrays


if __name__ == "__main__":
    torch.set_num_threads(1)
    ref = load_reference()
    for name, case in (("general", general_case), ("ties", ties_case), ("oblique", oblique_case), ("attrs", attrs_case)):
        path = os.path.join(HERE, f"tsdf_resample_{name}.npz")
        save_npz(path, case(ref))
        size = os.path.getsize(path)
        assert size < 1000000, (name, size)
        print(f"tsdf_resample_{name}.npz: {size} bytes")
