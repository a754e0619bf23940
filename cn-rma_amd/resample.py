"""TSDF resampling on the device: a TSDF volume and its attribute volumes read under a rigid transform into a new voxel grid
(csrc/resample.hip; reference: projects/mvsdetection/datasets/tsdf.py:112-180, TSDF.transform, and with attribute volumes
data_prepare/scannet/tsdf.py:266-349).

    out = resample_tsdf(tsdf, transform, voxel_dim, origin)          # projects.mvsdetection.datasets.tsdf.TSDF, on tsdf's device

The result equals TSDF.transform run on the CPU bit for bit, for every voxel (include/cnrma.h, a17, holds the arithmetic; the
matrix product is pinned as an un-fused sum from the left).  One gather kernel per volume, no device->host read.  Unlike the host
method, which squeezes, the output always has three axes [nx, ny, nz]."""
import math

import torch

from . import _lib
from ._lib import call, ptr, stream

INT_DTYPES = (torch.int64, torch.int32, torch.int16, torch.int8, torch.uint8)


def check_dims(src_dim, dst_dim):
    """what the entry points refuse, as a ValueError before anything is launched"""
    if len(src_dim) != 3 or len(dst_dim) != 3:
        raise ValueError(f"resample_tsdf wants volumes of three axes, got {tuple(src_dim)} -> {tuple(dst_dim)}")
    if min(src_dim) < 2:
        raise ValueError(f"resample_tsdf: every source dimension must be at least 2 (the grid is normalised by dim - 1), got "
                         f"{tuple(src_dim)}")
    if min(dst_dim) < 0 or math.prod(src_dim) >= 2 ** 31 or math.prod(dst_dim) >= 2 ** 31:
        raise ValueError(f"resample_tsdf wants volumes of fewer than 2^31 voxels, got {tuple(src_dim)} -> {tuple(dst_dim)}")


def resample_tsdf(tsdf, transform=None, voxel_dim=None, origin=None):
    """`tsdf` (a TSDF whose volumes live on a GPU) resampled under the rigid map `transform` (new world -> old world, 4x4 or 3x4;
    default: identity) into a volume of `voxel_dim` voxels (default: as the source) whose voxel (0,0,0) sits at `origin` (default:
    the source's): the same defaults as TSDF.transform.  tsdf_vol: nearest sample, trilinear inside the truncation band, +1
    outside the old volume.  Attribute volumes are carried along as the reference's data-preparation class does: float volumes
    ([X,Y,Z] or [C,X,Y,Z]) trilinear, integer volumes nearest, 'semseg' filled with -1 outside the old volume.  fp64 and
    non-contiguous inputs are converted.  -> a new TSDF on the source's device."""
    from projects.mvsdetection.datasets.tsdf import TSDF
    vol = tsdf.tsdf_vol
    src_dim = tuple(int(n) for n in vol.shape)
    dst_dim = src_dim if voxel_dim is None else tuple(int(n) for n in voxel_dim)
    check_dims(src_dim, dst_dim)
    for key, value in tsdf.attribute_vols.items():
        if tuple(value.shape[-3:]) != src_dim or value.dim() not in (3, 4):
            raise ValueError(f"resample_tsdf: attribute volume '{key}' of shape {tuple(value.shape)} does not go with a volume of "
                             f"{src_dim}")
        if not (value.dtype.is_floating_point or value.dtype in INT_DTYPES):
            raise ValueError(f"resample_tsdf: attribute volume '{key}' of {value.dtype} is not supported (float or integer volumes)")
    _lib.require_gpu()
    dev = vol.device
    T = torch.eye(4) if transform is None else torch.as_tensor(transform)
    if T.dim() != 2 or T.shape[0] not in (3, 4) or T.shape[1] != 4:
        raise ValueError(f"resample_tsdf wants a 4x4 or 3x4 transform, got shape {tuple(T.shape)}")
    # source origin [3], transform [3][4] and new origin [3] on the device; what is on the host crosses in one copy
    parts = [torch.as_tensor(tsdf.origin).reshape(3), T[:3].reshape(12),
             torch.as_tensor(tsdf.origin if origin is None else origin).reshape(3)]
    if all(p.device.type == "cpu" for p in parts):
        staged = torch.cat([p.to(torch.float32) for p in parts]).to(dev)
        src_origin, T, dst_origin = staged[:3], staged[3:15], staged[15:]
    else:
        src_origin, T, dst_origin = (p.to(dev, torch.float32).contiguous() for p in parts)
    new_origin = tsdf.origin if origin is None else dst_origin.view(1, 3)
    X, Y, Z = src_dim
    nx, ny, nz = dst_dim
    vs = float(tsdf.voxel_size)
    geometry = (ptr(src_origin), vs, ptr(T), ptr(dst_origin), nx, ny, nz)

    out = torch.empty(dst_dim, dtype=torch.float32, device=dev)
    call("cnrma_tsdf_resample_f32", ptr(vol.to(torch.float32).contiguous()), X, Y, Z, *geometry, ptr(out), stream())
    attrs = {}
    for key, value in tsdf.attribute_vols.items():
        lead = tuple(value.shape[:-3])
        C = lead[0] if lead else 1
        if value.dtype.is_floating_point:
            res = torch.empty(lead + dst_dim, dtype=torch.float32, device=dev)
            call("cnrma_tsdf_resample_attr_f32", ptr(value.to(torch.float32).contiguous()), C, X, Y, Z, *geometry, ptr(res), stream())
        else:
            res = torch.empty(lead + dst_dim, dtype=torch.int64, device=dev)
            call("cnrma_tsdf_resample_attr_i64", ptr(value.to(torch.int64).contiguous()), C, X, Y, Z, *geometry, -1,
                 1 if key == "semseg" else 0, ptr(res), stream())
        attrs[key] = res.to(value.dtype)
    return TSDF(tsdf.voxel_size, new_origin, out, attrs)
