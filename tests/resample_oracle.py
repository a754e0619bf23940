"""Host oracle of the TSDF resampling (cnrma_amd.resample / csrc/resample.hip): the arithmetic of include/cnrma.h (a17) restated in
torch on the CPU with elementwise operations only -- no matrix product and no grid_sample --, one full-volume expression per step,
every choice a torch.where.  tests/golden/make_golden_resample.py asserts that it equals TSDF.transform on the CPU (the reference's
and the project's) bit for bit; the tests then use it wherever no fixture exists.

    pos = positions(src_dim, src_origin, voxel_size, transform, dst_dim, dst_origin)
    vol = resample_volume(src, pos)        attr = resample_float(src_c, pos)        lab = resample_int(src_i, pos, fill=None)

Volumes come back as [nx, ny, nz] ([C, nx, ny, nz] for a channelled source).  All arithmetic is float32."""
import torch


def f32(x):
    return torch.tensor(float(x), dtype=torch.float32)


def positions(src_dim, src_origin, voxel_size, transform, dst_dim, dst_origin):
    """-> dict(s=[3, N] source positions in grid_sample's pixel units (volume x, y, z), n=[3, N] normalised coordinates,
    border=[N] bool, src_dim, dst_dim); N = nx ny nz, index (x ny + y) nz + z"""
    nx, ny, nz = (int(d) for d in dst_dim)
    g = torch.arange(nx * ny * nz, dtype=torch.long)
    idx = torch.stack((g // (ny * nz), (g // nz) % ny, g % nz)).float()
    vs = f32(voxel_size)
    do = torch.as_tensor(dst_origin, dtype=torch.float32).reshape(3)
    so = torch.as_tensor(src_origin, dtype=torch.float32).reshape(3)
    T = torch.as_tensor(transform, dtype=torch.float32)[:3]
    w = [idx[a] * vs + do[a] for a in range(3)]                                   # two roundings
    s, n = [], []
    border = torch.zeros(nx * ny * nz, dtype=torch.bool)
    for a in range(3):
        p = ((T[a, 0] * w[0] + T[a, 1] * w[1]) + T[a, 2] * w[2]) + T[a, 3] * f32(1)          # un-fused, from the left
        c = (p - so[a]) / vs
        na = f32(2) * c / f32(int(src_dim[a]) - 1) - f32(1)
        border = border | (na.abs() >= 1)                                         # a NaN compares false
        s.append(((na + f32(1)) * f32(int(src_dim[a])) - f32(1)) / f32(2))
        n.append(na)
    return dict(s=torch.stack(s), n=torch.stack(n), border=border, src_dim=tuple(int(d) for d in src_dim), dst_dim=(nx, ny, nz))


def _gather(flat, pos_xyz, dims):
    """flat [C, S] at float indices pos_xyz (three [N] tensors of integral values or anything else) -> (values [C, N], inside [N]);
    the address of an index outside the volume is clamped and its value must not be used"""
    inside = torch.ones_like(pos_xyz[0], dtype=torch.bool)
    lin = torch.zeros_like(pos_xyz[0], dtype=torch.long)
    for a in range(3):
        f = pos_xyz[a]
        inside = inside & (f >= 0) & (f < dims[a])                                # NaN and +-inf fail
        safe = torch.where((f >= 0) & (f < dims[a]), f, torch.zeros_like(f)).long()
        lin = lin * dims[a] + safe
    return flat[:, lin], inside


def nearest(src, pos):
    """[C, X, Y, Z] (any dtype) -> [C, N]: rint with ties to even, zero outside the volume"""
    dims = pos["src_dim"]
    flat = src.reshape(src.shape[0], -1)
    v, inside = _gather(flat, [torch.round(pos["s"][a]) for a in range(3)], dims)
    return torch.where(inside.unsqueeze(0), v, torch.zeros_like(v))


def trilinear(src, pos):
    """[C, X, Y, Z] float32 -> [C, N]: ATen's corner order (z offset fastest), weight product (wz wy) wx, sum from +0 over the
    corners inside the volume"""
    dims = pos["src_dim"]
    flat = src.reshape(src.shape[0], -1)
    s = pos["s"]
    f = [torch.floor(s[a]) for a in range(3)]
    wt = [((f[a] + f32(1)) - s[a], s[a] - f[a]) for a in range(3)]
    acc = torch.zeros(flat.shape[0], s.shape[1], dtype=torch.float32)
    for dx in (0, 1):
        for dy in (0, 1):
            for dz in (0, 1):
                v, inside = _gather(flat, [f[0] + f32(dx), f[1] + f32(dy), f[2] + f32(dz)], dims)
                weight = (wt[2][dz] * wt[1][dy]) * wt[0][dx]
                acc = torch.where(inside.unsqueeze(0), acc + v * weight.unsqueeze(0), acc)
    return acc


def resample_volume(src, pos):
    """the TSDF volume [X, Y, Z]: nearest, trilinear inside the band |nearest| < 1, +1 on the border"""
    src = src.float().reshape((1,) + tuple(pos["src_dim"]))
    near, lin = nearest(src, pos)[0], trilinear(src, pos)[0]
    out = torch.where(near.abs() < 1, lin, near)
    out = torch.where(pos["border"], torch.ones_like(out), out)
    return out.view(pos["dst_dim"])


def resample_float(src, pos):
    """a float attribute volume [X, Y, Z] or [C, X, Y, Z]: trilinear with zero padding"""
    lead = tuple(src.shape[:-3])
    out = trilinear(src.float().reshape((-1,) + tuple(pos["src_dim"])), pos)
    return out.view(lead + pos["dst_dim"])


def resample_int(src, pos, fill=None):
    """an integer attribute volume [X, Y, Z] or [C, X, Y, Z]: nearest with zero padding, gathered as integers; fill: the value of
    border voxels (None: as sampled)"""
    lead = tuple(src.shape[:-3])
    out = nearest(src.reshape((-1,) + tuple(pos["src_dim"])), pos)
    if fill is not None:
        out = torch.where(pos["border"].unsqueeze(0), torch.full_like(out, fill), out)
    return out.view(lead + pos["dst_dim"])


def resample_tsdf_oracle(tsdf, transform=None, voxel_dim=None, origin=None):
    """tsdf: anything with voxel_size, origin, tsdf_vol, attribute_vols (CPU) -> (volume, {name: attribute volume}), with
    TSDF.transform's defaults"""
    src_dim = tuple(tsdf.tsdf_vol.shape)
    T = torch.eye(4) if transform is None else transform
    dst_dim = src_dim if voxel_dim is None else tuple(voxel_dim)
    dst_origin = tsdf.origin if origin is None else torch.tensor(origin, dtype=torch.float)
    pos = positions(src_dim, tsdf.origin, tsdf.voxel_size, T, dst_dim, dst_origin)
    attrs = {}
    for key, value in getattr(tsdf, "attribute_vols", {}).items():
        if value.dtype.is_floating_point:
            attrs[key] = resample_float(value, pos)
        else:
            attrs[key] = resample_int(value, pos, fill=-1 if key == "semseg" else None)
    return resample_volume(tsdf.tsdf_vol, pos), attrs
