"""TSDF fusion on the device: posed depth maps (and colour / label images) accumulated into a TSDF volume (csrc/fusion.hip;
reference: data_prepare/scannet/tsdf.py:353-474, TSDFFusion, which generate_tsdf.py:104-126 feeds one frame at a time).

    fusion = TSDFFusion(voxel_dim, voxel_size, origin, color=True)
    fusion.integrate(projections, depths, colors)          # [V,3,4], [V,H,W], [V,3,H,W]: one launch for the whole batch
    tsdf = fusion.get_tsdf()                               # projects.mvsdetection.datasets.tsdf.TSDF
    tsdf.save("tsdf_04.npz")

The result equals the reference's TSDFFusion run on the CPU bit for bit, for every voxel (include/cnrma.h, a16, holds the
arithmetic).  The volumes cross memory once per integrate() call, so frames are best fed in batches."""
import math

import torch

from . import _lib
from ._lib import call, ptr, stream


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
