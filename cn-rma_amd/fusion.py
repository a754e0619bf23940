"""TSDF fusion on the device: posed depth maps (and colour / label images) accumulated into a TSDF volume (csrc/fusion.hip;
reference: data_prepare/scannet/tsdf.py:353-474, TSDFFusion, which generate_tsdf.py:104-126 feeds one frame at a time).

    fusion = TSDFFusion(voxel_dim, voxel_size, origin, color=True)
    fusion.integrate(projections, depths, colors)          # [V,3,4], [V,H,W], [V,3,H,W]: one launch for the whole batch
    tsdf = fusion.get_tsdf()                               # projects.mvsdetection.datasets.tsdf.TSDF
    tsdf.save("tsdf_04.npz")

The result equals the reference's TSDFFusion run on the CPU bit for bit, for every voxel (include/cnrma.h, a16, holds the
arithmetic).  The volumes cross memory once per integrate() call, so frames are best fed in batches.

Where the volume lies is found on the device as well (csrc/bounds.hip; reference: generate_tsdf.py:82-101, a point cloud of up to 200
back-projected depth maps copied to the host and two np.quantile):

    origin, voxel_dim = scene_bounds(projections, depths, voxel_size, max_depth=3.)      # float32 CPU tensor [3], [nx, ny, nz]
    tsdf = fuse_scene(projections, depths, colors, voxel_size=.04)                       # bounds, integrate, get_tsdf in one call

Both equal the reference's host arithmetic bit for bit (include/cnrma_prep.h, p1)."""
import math

import numpy as np
import torch

from . import _lib
from ._lib import call, call_prep, ptr, stream


class TSDFFusion:
    def __init__(self, voxel_dim=(128, 128, 128), voxel_size=.02, origin=(0, 0, 0), trunc_ratio=3, device=None, color=True,
                 label=False):
        """voxel_dim (nx, ny, nz), voxel_size in metres, origin = position of voxel (0,0,0), trunc_ratio = voxels before the
        distance is truncated to 1; color / label: also accumulate an RGB volume / a label volume.  device: default cuda."""
        voxel_dim = tuple(int(n) for n in voxel_dim)
        if len(voxel_dim) != 3 or min(voxel_dim) < 0 or math.prod(voxel_dim) >= 2 ** 31:
            raise ValueError(f"TSDFFusion wants voxel_dim (nx, ny, nz) with fewer than 2^31 voxels, got {voxel_dim}")
        self.voxel_dim = voxel_dim
        self.voxel_size = voxel_size
        self.trunc_margin = voxel_size * trunc_ratio                  # a Python float; rounded to fp32 once, at the call
        self.device = torch.device("cuda" if device is None else device)
        self.origin = torch.as_tensor(origin, dtype=torch.float32).reshape(1, 3).to(self.device)
        n = math.prod(voxel_dim)
        self.tsdf_vol = torch.empty(n, dtype=torch.float32, device=self.device)
        self.weight_vol = torch.empty(n, dtype=torch.float32, device=self.device)
        self.color_vol = torch.empty((3, n), dtype=torch.float32, device=self.device) if color else None
        self.label_vol = torch.empty(n, dtype=torch.int32, device=self.device) if label else None
        self.reset()

    def reset(self):
        """the initial state: tsdf 1, weight 0, colour 0, label -1"""
        self.tsdf_vol.fill_(1)
        self.weight_vol.fill_(0)
        if self.color_vol is not None:
            self.color_vol.fill_(0)
        if self.label_vol is not None:
            self.label_vol.fill_(-1)

    def integrate(self, projection, depth, color=None, label=None, max_depth=None):
        """Accumulate one view -- projection [3,4] (intrinsics @ extrinsics), depth [H,W], color [3,H,W], label [H,W] -- or a batch
        of V views ([V,3,4], [V,H,W], [V,3,H,W], [V,H,W]) fused in index order by one launch.  Depths above max_depth count as
        missing (generate_tsdf.py:119).  color is needed when the fusion keeps a colour volume, label when it keeps labels; an
        image the fusion keeps no volume for is ignored, as in the reference.  No device->host read."""
        projection, depth = torch.as_tensor(projection), torch.as_tensor(depth)
        if projection.dim() == 2:
            lead = ()
        elif projection.dim() == 3:
            lead = (int(projection.shape[0]),)
        else:
            raise ValueError(f"integrate wants a [3,4] or [V,3,4] projection, got shape {tuple(projection.shape)}")
        if tuple(projection.shape[-2:]) != (3, 4):
            raise ValueError(f"integrate wants a [3,4] or [V,3,4] projection, got shape {tuple(projection.shape)}")
        if depth.dim() != len(lead) + 2 or tuple(depth.shape[:len(lead)]) != lead:
            raise ValueError(f"integrate: depth of shape {tuple(depth.shape)} does not go with a projection of shape "
                             f"{tuple(projection.shape)} (one view: [H,W]; a batch: [V,H,W])")
        H, W = int(depth.shape[-2]), int(depth.shape[-1])
        if H >= 2 ** 24 or W >= 2 ** 24:
            raise ValueError(f"integrate: images of {H} x {W} pixels are not supported (each side < 2^24)")
        if self.color_vol is None:
            color = None
        elif color is None:
            raise ValueError("integrate: this fusion accumulates colour (color=True): pass the colour image")
        else:
            color = torch.as_tensor(color)
            if tuple(color.shape) != lead + (3, H, W):
                raise ValueError(f"integrate: color of shape {tuple(color.shape)}, expected {lead + (3, H, W)}")
        if self.label_vol is None:
            label = None
        elif label is None:
            raise ValueError("integrate: this fusion accumulates labels (label=True): pass the label image")
        else:
            label = torch.as_tensor(label)
            if tuple(label.shape) != lead + (H, W):
                raise ValueError(f"integrate: label of shape {tuple(label.shape)}, expected {lead + (H, W)}")
        _lib.require_gpu()
        dev = self.device
        V = lead[0] if lead else 1
        projection = projection.to(dev, torch.float32).contiguous()
        depth = depth.to(dev, torch.float32).contiguous()
        if color is not None:
            color = color.to(dev, torch.float32).contiguous()
        if label is not None:
            label = label.to(dev, torch.int32).contiguous()
        X, Y, Z = self.voxel_dim
        call("cnrma_tsdf_fuse_f32", ptr(projection), ptr(depth), ptr(color), ptr(label), ptr(self.origin), V, H, W, X, Y, Z,
             float(self.voxel_size), float(self.trunc_margin), math.inf if max_depth is None else float(max_depth),
             ptr(self.tsdf_vol), ptr(self.weight_vol), ptr(self.color_vol), ptr(self.label_vol), stream())

    def get_tsdf(self, label_name="instance"):
        """The fused volume as a TSDF (sums divided by the weights where a voxel was observed): tsdf_vol [nx,ny,nz],
        attribute_vols['color'] [3,nx,ny,nz], attribute_vols[label_name] [nx,ny,nz] int64.  The running volumes stay as they are:
        integration can go on afterwards."""
        from projects.mvsdetection.datasets.tsdf import TSDF
        _lib.require_gpu()
        X, Y, Z = self.voxel_dim
        n = X * Y * Z
        tsdf_vol = torch.empty_like(self.tsdf_vol)
        color_vol = None if self.color_vol is None else torch.empty_like(self.color_vol)
        call("cnrma_tsdf_fuse_finish_f32", ptr(self.tsdf_vol), ptr(self.weight_vol), ptr(self.color_vol), n, ptr(tsdf_vol),
             ptr(color_vol), stream())
        attribute_vols = {}
        if color_vol is not None:
            attribute_vols["color"] = color_vol.view(3, X, Y, Z)
        if self.label_vol is not None:
            attribute_vols[label_name] = self.label_vol.view(X, Y, Z).long()
        return TSDF(self.voxel_size, self.origin, tsdf_vol.view(X, Y, Z), attribute_vols)


def _lerp(a, b, t):
    """numpy's linear interpolation between the two order statistics (numpy/lib/_function_base_impl.py, _lerp), all float32"""
    diff = np.subtract(b, a)
    out = np.asanyarray(np.add(a, diff * t))
    np.subtract(b, diff * (1 - t), out=out, where=t >= 0.5, casting="unsafe", dtype=type(out.dtype))
    return out


def quantile_finish(lo, hi, n, q, nans):
    """np.quantile(pts, q, axis=0) of a float32 sample of n rows from its order statistics lo = s[k], hi = s[k1] per axis ([3] float32
    each) and the number of NaNs per axis: what numpy (2.x, method 'linear') does after its partition.  q is a Python float, which
    numpy takes to the sample's float32, so the virtual index (n - 1) * q and the weight are float32 as well."""
    q = np.asanyarray(q, dtype=np.float32)
    vi = np.asanyarray((n - 1) * q)
    k = np.floor(vi)
    if vi >= n - 1:                                     # numpy indexes the last element as -1 there, and forms the weight from that
        k = np.float32(-1)
    gamma = np.asanyarray(vi - k.astype(np.intp), dtype=np.float32).reshape(1)
    out = _lerp(np.asarray(lo, np.float32), np.asarray(hi, np.float32), gamma)
    out[np.asarray(nans) > 0] = np.nan                  # a NaN sorts last, and numpy hands it out for the whole axis
    return out


def _check_views(name, projections, depths):
    if projections.dim() != 3 or tuple(projections.shape[1:]) != (3, 4):
        raise ValueError(f"{name} wants projections of shape [V,3,4], got {tuple(projections.shape)}")
    if depths.dim() != 3 or depths.shape[0] != projections.shape[0]:
        raise ValueError(f"{name}: depths of shape {tuple(depths.shape)} do not go with projections of shape "
                         f"{tuple(projections.shape)} (wanted [V,H,W])")
    if depths.numel() >= 2 ** 31:
        raise ValueError(f"{name}: {depths.numel()} depth pixels are not supported (fewer than 2^31)")


def scene_bounds(projections, depths, voxel_size, max_depth=None, vol_prcnt=.995, vol_margin=1.5, device=None, pinv=None):
    """Where the fusion volume of these views lies (generate_tsdf.py:82-101): projections [V,3,4] (intrinsics @ extrinsics), depths
    [V,H,W] -> (origin: float32 CPU tensor [3], voxel_dim: [nx, ny, nz]).  Every depth pixel is back-projected (depths above max_depth
    count as missing), the points with a finite x are kept, origin = their (1 - vol_prcnt) quantile per axis - vol_margin, the far
    corner their vol_prcnt quantile + vol_margin.  The points are never stored: the device selects the order statistics exactly and
    the host interpolates as numpy does.  The matrix inverses are taken on the host, one torch.inverse per view (pass the projections
    as CPU tensors); pinv [V,4,4] replaces them when given (LAPACK's inverse is not bit-stable across host CPUs: a result recorded
    elsewhere is reproduced bit for bit only from the inverses recorded with it).  ONE device->host read, of 80 bytes.  Raises
    ValueError when no pixel has a usable depth."""
    projections, depths = torch.as_tensor(projections), torch.as_tensor(depths)
    _check_views("scene_bounds", projections, depths)
    vol_prcnt = float(vol_prcnt)
    if not 0. <= vol_prcnt <= 1.:
        raise ValueError(f"scene_bounds wants 0 <= vol_prcnt <= 1, got {vol_prcnt}")
    if not voxel_size > 0:
        raise ValueError(f"scene_bounds wants a positive voxel_size, got {voxel_size}")
    if pinv is not None:
        pinv = torch.as_tensor(pinv)
        if tuple(pinv.shape) != (int(projections.shape[0]), 4, 4):
            raise ValueError(f"scene_bounds: pinv of shape {tuple(pinv.shape)}, expected {(int(projections.shape[0]), 4, 4)}")
    _lib.require_gpu()
    dev = torch.device("cuda" if device is None else device)
    V, H, W = (int(s) for s in depths.shape)
    if pinv is None:
        eye_row = torch.tensor([[0., 0., 0., 1.]])
        host = projections.to("cpu", torch.float32)
        pinv = torch.stack([torch.inverse(torch.cat((P, eye_row))) for P in host]) if V else torch.zeros(0, 4, 4)
    pinv = pinv.to(dev, torch.float32).contiguous()
    depths = depths.to(dev, torch.float32).contiguous()
    q_lo, q_hi = 1 - vol_prcnt, vol_prcnt
    out = torch.zeros(10, dtype=torch.int64, device=dev)              # [4] counts, then [2][3][2] float32 values
    nbytes = _lib.load_prep().cnrma_prep_bounds_workspace_bytes()
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    call_prep("cnrma_prep_depth_bounds_f32", ptr(pinv) if V else None, ptr(depths) if depths.numel() else None, V, H, W,
              math.inf if max_depth is None else float(max_depth), q_lo, q_hi, ptr(ws), nbytes, out.data_ptr() + 32, ptr(out), stream())
    got = out.cpu()                                                    # the one read
    n, nans = int(got[0]), got[1:4].numpy()
    if n == 0:
        raise ValueError("no pixel with a usable depth")
    values = got[4:].view(torch.float32).numpy().reshape(2, 3, 2)
    lo = quantile_finish(values[0, :, 0], values[0, :, 1], n, q_lo, nans)
    hi = quantile_finish(values[1, :, 0], values[1, :, 1], n, q_hi, nans)
    origin = torch.as_tensor(lo - vol_margin).float()                  # generate_tsdf.py:99-101, on CPU tensors
    vol_max = torch.as_tensor(hi + vol_margin).float()
    voxel_dim = ((vol_max - origin) / voxel_size).int().tolist()
    return origin, voxel_dim


def fuse_scene(projections, depths, colors=None, voxel_size=.04, trunc_ratio=3, max_depth=3., vol_prcnt=.995, vol_margin=1.5,
               batch=32, device=None):
    """The reference's fuse_scene (generate_tsdf.py:82-126) in one call: the bounds from all frames (from 200 evenly spaced ones when
    there are more), a TSDFFusion of that volume without labels -- with colour when colors [V,3,H,W] is given --, every frame
    integrated in index order, `batch` per launch, with depths above max_depth masked, and get_tsdf()."""
    projections, depths = torch.as_tensor(projections), torch.as_tensor(depths)
    _check_views("fuse_scene", projections, depths)
    if colors is not None:
        colors = torch.as_tensor(colors)
    if int(batch) < 1:
        raise ValueError(f"fuse_scene wants batch >= 1, got {batch}")
    n = int(projections.shape[0])
    if n <= 200:
        origin, voxel_dim = scene_bounds(projections, depths, voxel_size, max_depth, vol_prcnt, vol_margin, device)
    else:
        inds = torch.as_tensor(np.linspace(0, n - 1, 200).astype(int))
        origin, voxel_dim = scene_bounds(projections[inds], depths[inds.to(depths.device)], voxel_size, max_depth, vol_prcnt, vol_margin,
                                         device)
    fusion = TSDFFusion(voxel_dim, voxel_size, origin, trunc_ratio, device, color=colors is not None, label=False)
    for s in range(0, n, int(batch)):
        e = s + int(batch)
        fusion.integrate(projections[s:e], depths[s:e], None if colors is None else colors[s:e], max_depth=max_depth)
    return fusion.get_tsdf()
