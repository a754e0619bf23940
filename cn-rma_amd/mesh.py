"""Mesh of a TSDF volume on the device: marching cubes (csrc/mesh.hip; reference: datasets/tsdf.py:81-114, TSDF.get_mesh, which
needs scikit-image and trimesh on the host).

    mesh = marching_cubes(tsdf_vol, voxel_size, origin)      # device tensors: vertices, faces, vertex_normals
    mesh.export("scene.ply")

The field is the reference's (unobserved voxels v == 1 count as inside, -v clamped to [-1, 1], level 0) and so is its empty
rule.  The triangulation is the classic marching cubes with the generated case table of cnrma_amd.mesh_table, whose face rule
keeps neighbouring cells consistent -- NOT scikit-image's Lewiner variant, which resolves ambiguous cases with interior tests
and extra vertices: the meshes do not match triangle for triangle.  Edge vertices are the same linear interpolation.  Vertex
and face order are fixed (owner voxel then axis; cell then table order), so the mesh is reproducible bit for bit."""
import os

import numpy as np
import torch

from . import _lib
from ._lib import call, ptr, stream

_PLY_VERTEX = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4")])
_PLY_FACE = np.dtype([("n", "u1"), ("v", "<i4", (3,))])


class Mesh:
    """vertices [Nv,3] float32, faces [Nf,3] int32 (counter-clockwise seen from outside), vertex_normals [Nv,3] float32"""

    def __init__(self, vertices, faces, vertex_normals):
        self.vertices, self.faces, self.vertex_normals = vertices, faces, vertex_normals

    def cpu(self):
        return Mesh(self.vertices.cpu(), self.faces.cpu(), self.vertex_normals.cpu())

    def export(self, path):
        """binary little-endian PLY: x y z nx ny nz as float32, faces as `list uchar int vertex_indices` (the layout of
        trimesh's export of such a mesh); written under a temporary name and renamed into place"""
        v = self.vertices.detach().cpu().numpy().astype("<f4", copy=False).reshape(-1, 3)
        n = self.vertex_normals.detach().cpu().numpy().astype("<f4", copy=False).reshape(-1, 3)
        f = self.faces.detach().cpu().numpy().astype("<i4", copy=False).reshape(-1, 3)
        vert = np.empty(len(v), dtype=_PLY_VERTEX)
        for k, name in enumerate(("x", "y", "z")):
            vert[name] = v[:, k]
            vert["n" + name] = n[:, k]
        face = np.empty(len(f), dtype=_PLY_FACE)
        face["n"] = 3
        face["v"] = f
        header = ("ply\nformat binary_little_endian 1.0\n"
                  f"element vertex {len(v)}\n"
                  "property float x\nproperty float y\nproperty float z\nproperty float nx\nproperty float ny\nproperty float nz\n"
                  f"element face {len(f)}\n"
                  "property list uchar int vertex_indices\nend_header\n")
        tmp = f"{path}.tmp{os.getpid()}"
        with open(tmp, "wb") as fh:
            fh.write(header.encode("ascii"))
            fh.write(vert.tobytes())
            fh.write(face.tobytes())
        os.replace(tmp, path)                      # a reader (or a crash) never sees a half-written file


def marching_cubes(tsdf_vol, voxel_size=1.0, origin=None):
    """Mesh of the device tensor tsdf_vol [X,Y,Z] (anything but float32 is widened with .float()); `origin` (3 numbers or a
    tensor, default 0) is the position of voxel (0,0,0).  Runs on the current stream; ONE device->host read (the counts)
    sizes the outputs exactly."""
    _lib.require_gpu()
    if tsdf_vol.dim() != 3:
        raise ValueError(f"marching_cubes wants a [X,Y,Z] volume, got shape {tuple(tsdf_vol.shape)}")
    vol = tsdf_vol.detach().float().contiguous()
    dev = vol.device
    X, Y, Z = (int(s) for s in vol.shape)
    if origin is None:
        org = torch.zeros(3, dtype=torch.float32, device=dev)
    else:
        org = torch.as_tensor(origin, dtype=torch.float32).reshape(3).to(dev).contiguous()
    ws = _lib.scratch("cnrma_mesh_workspace_bytes", X, Y, Z, device=dev)
    if ws.numel() == 0:
        raise _lib.CnrmaError(f"marching_cubes: unsupported volume shape {(X, Y, Z)}")
    counts = torch.empty(4, dtype=torch.int32, device=dev)
    call("cnrma_mesh_count_f32", ptr(vol), X, Y, Z, ptr(ws), ws.numel(), ptr(counts), stream())
    nv, nf = _lib.read_ints(counts)[:2]
    vertices = torch.empty((nv, 3), dtype=torch.float32, device=dev)
    normals = torch.empty((nv, 3), dtype=torch.float32, device=dev)
    faces = torch.empty((nf, 3), dtype=torch.int32, device=dev)
    if nv or nf:
        call("cnrma_mesh_emit_f32", ptr(vol), X, Y, Z, float(voxel_size), ptr(org), ptr(ws), ptr(vertices), ptr(normals), nv,
             ptr(faces), nf, ptr(counts), stream())
    return Mesh(vertices, faces, normals)
