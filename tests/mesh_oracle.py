"""Host oracle of the device mesh extraction (cnrma_amd.mesh / csrc/mesh.hip): a numpy marching cubes, vectorised over the
active cells, with the conventions and the case table of cnrma_amd.mesh_table and the kernels' float32 expression order.

    field        g = 1 where v == 1, else clip(-v, -1, 1)            (reference datasets/tsdf.py:95-104)
    empty        no voxel with g < 0, or none with g > 0             (reference tsdf.py:106-107: min >= 0 or max <= 0)
    inside       g > 0
    vertex       one per sign-change edge, owned by the edge's lower voxel; order: owner (x Y + y) Z + z, then axis
                 t = g0 / (g0 - g1);  p = owner index, + t on the edge's axis;  world = p * voxel_size + origin
    normal       gradient of g at both edge ends (central differences * 0.5, one-sided at the border), n = n0 + t * (n1 - n0),
                 negated, divided by sqrt((nx nx + ny ny) + nz nz); (0, 0, 0) when that is 0
    faces        active cells by linear index, then table order

The helpers below the extraction (edge statistics, signed volume, sign-change count) do not use the table."""
import numpy as np

from cnrma_amd import mesh_table

F = np.float32
_NTRI = np.array([len(t) for t in mesh_table.TABLE], dtype=np.int64)
_TRI = np.zeros((256, 15), dtype=np.int64)
for _c, _t in enumerate(mesh_table.TABLE):
    _flat = [e for tri in _t for e in tri]
    _TRI[_c, :len(_flat)] = _flat
_EDGE_AXIS = np.arange(12) // 4
_EDGE_START = np.array([mesh_table.corner_offset(mesh_table.EDGES[e][0]) for e in range(12)], dtype=np.int64)   # [12, 3]


def field(v):
    v = np.asarray(v, dtype=F)
    return np.where(v == 1, F(1), np.clip(-v, F(-1), F(1))).astype(F)


def _gradient(g):
    """[X,Y,Z,3] float32: central differences * 0.5 inside, one-sided at the border, 0 along an axis of length 1"""
    out = np.zeros(g.shape + (3,), dtype=F)
    for a in range(3):
        n = g.shape[a]
        if n < 2:
            continue
        gm = np.moveaxis(g, a, 0)
        d = np.empty_like(gm)
        d[1:-1] = (gm[2:] - gm[:-2]) * F(0.5)
        d[0] = gm[1] - gm[0]
        d[-1] = gm[-1] - gm[-2]
        out[..., a] = np.moveaxis(d, 0, a)
    return out


def marching_cubes(tsdf, voxel_size=1.0, origin=None):
    """-> dict(vertices [Nv,3] f32, normals [Nv,3] f32, faces [Nf,3] i32, counts (n_vertices, n_triangles, n_active_cells))"""
    g = field(tsdf)
    X, Y, Z = g.shape
    origin = np.zeros(3, dtype=F) if origin is None else np.asarray(origin, dtype=F).reshape(3)
    empty = dict(vertices=np.zeros((0, 3), F), normals=np.zeros((0, 3), F), faces=np.zeros((0, 3), np.int32), counts=(0, 0, 0))
    if min(X, Y, Z) < 2 or not (g < 0).any() or not (g > 0).any():
        return empty
    ins = g > 0
    # ---- vertices: the owned edges with a sign change, in (voxel, axis) order
    own = np.zeros((X, Y, Z, 3), dtype=bool)
    own[:-1, :, :, 0] = ins[:-1] != ins[1:]
    own[:, :-1, :, 1] = ins[:, :-1] != ins[:, 1:]
    own[:, :, :-1, 2] = ins[:, :, :-1] != ins[:, :, 1:]
    vid = (np.cumsum(own.reshape(-1)) - 1).reshape(X, Y, Z, 3)
    x, y, z, a = np.nonzero(own)
    e = np.eye(3, dtype=np.int64)[a]
    g0, g1 = g[x, y, z], g[x + e[:, 0], y + e[:, 1], z + e[:, 2]]
    t = (g0 / (g0 - g1)).astype(F)
    p = np.stack((x, y, z), axis=1).astype(F)
    p[np.arange(len(a)), a] += t
    vertices = (p * F(voxel_size) + origin[None]).astype(F)
    grad = _gradient(g)
    n0, n1 = grad[x, y, z], grad[x + e[:, 0], y + e[:, 1], z + e[:, 2]]
    n = -(n0 + t[:, None] * (n1 - n0)).astype(F)
    length = np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2]).astype(F)
    normals = np.where(length[:, None] > 0, n / np.where(length > 0, length, F(1))[:, None], F(0)).astype(F)
    # ---- faces: the active cells in linear order, table order inside a cell
    case = np.zeros((X - 1, Y - 1, Z - 1), dtype=np.int64)
    for i in range(8):
        dx, dy, dz = mesh_table.corner_offset(i)
        case |= ins[dx:X - 1 + dx, dy:Y - 1 + dy, dz:Z - 1 + dz].astype(np.int64) << i
    cx, cy, cz = np.nonzero((case != 0) & (case != 255))
    cc = case[cx, cy, cz]
    ntri = _NTRI[cc]
    rep = np.repeat(np.arange(len(cc)), ntri)
    k = np.arange(len(rep)) - np.repeat(np.cumsum(ntri) - ntri, ntri)                  # triangle number inside its cell
    edges = _TRI[cc[rep][:, None], 3 * k[:, None] + np.arange(3)[None]]                # [Nf, 3] edge ids
    s = _EDGE_START[edges]
    faces = vid[cx[rep][:, None] + s[..., 0], cy[rep][:, None] + s[..., 1], cz[rep][:, None] + s[..., 2], _EDGE_AXIS[edges]]
    return dict(vertices=vertices, normals=normals, faces=faces.astype(np.int32), counts=(len(vertices), len(faces), len(cc)))


# ---- table-free checks ------------------------------------------------------------------------------------------------------
def sign_change_edges(g):
    """number of grid edges whose ends differ in `g > 0` (g: the transformed field)"""
    ins = np.asarray(g) > 0
    return int((ins[:-1] != ins[1:]).sum() + (ins[:, :-1] != ins[:, 1:]).sum() + (ins[:, :, :-1] != ins[:, :, 1:]).sum())


def edge_stats(faces):
    """(number of directed edges that occur more than once, the directed edges [K,2] that occur more often than their
    opposite).  Inside one cell every directed edge occurs once; in a whole mesh a fan diagonal that lies in a cell face can
    coincide with an edge of the neighbour cell, so there an edge may occur twice -- with its opposite twice as well."""
    f = np.asarray(faces, dtype=np.int64)
    d = np.concatenate((f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]))
    if len(d) == 0:
        return 0, np.zeros((0, 2), np.int64)
    m = int(f.max()) + 1
    key, cnt = np.unique(d[:, 0] * m + d[:, 1], return_counts=True)
    okey, ocnt = np.unique(d[:, 1] * m + d[:, 0], return_counts=True)
    have = dict(zip(okey.tolist(), ocnt.tolist()))
    more = np.array([c > have.get(k, 0) for k, c in zip(key.tolist(), cnt.tolist())], dtype=bool)
    return int((cnt > 1).sum()), np.stack((key[more] // m, key[more] % m), axis=1)


def is_closed_and_oriented(faces):
    """every directed edge is matched by its opposite"""
    return len(edge_stats(faces)[1]) == 0


def signed_volume(vertices, faces):
    """float64; positive when the triangles are counter-clockwise seen from outside the enclosed ("inside") region"""
    v = np.asarray(vertices, dtype=np.float64)[np.asarray(faces, dtype=np.int64)]
    return float(np.einsum("ij,ij->i", v[:, 0], np.cross(v[:, 1], v[:, 2])).sum() / 6.0)


def euler_characteristic(n_vertices, faces):
    f = np.asarray(faces, dtype=np.int64)
    e = np.unique(np.sort(np.concatenate((f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]])), axis=1), axis=0)
    return int(n_vertices) - len(e) + len(f)


def tsdf_of_field(g):
    """a TSDF volume v with field(v) == g, for g in [-1, 1]: v = -g, and v = 2 where g == -1 (v = 1 would be the reference's
    "unobserved" marker, which the field turns into +1; 2 clips to g = -1)"""
    g = np.asarray(g, dtype=F)
    assert (g <= 1).all() and (g >= -1).all()
    return np.where(g == -1, F(2), -g).astype(F)


def shelled(g):
    """g with its outermost voxel layer set to -1 (outside): every surface then closes inside the volume"""
    g = np.array(g, dtype=F)
    g[[0, -1]] = -1
    g[:, [0, -1]] = -1
    g[:, :, [0, -1]] = -1
    return g


def case_block(case, rng):
    """the field g of a 4x4x4 volume whose central cell has `case`: shell and outside corners -1, inside corners drawn
    from (0.1, 1)"""
    g = np.full((4, 4, 4), -1.0, dtype=F)
    for i in range(8):
        if (case >> i) & 1:
            dx, dy, dz = mesh_table.corner_offset(i)
            g[1 + dx, 1 + dy, 1 + dz] = min(F(rng.uniform(0.1, 1.0)), F(0.999))
    return g


def read_ply(path):
    """minimal reader of the binary PLY that cnrma_amd.mesh.Mesh.export writes -> (vertices [Nv,3] f32, normals [Nv,3] f32,
    faces [Nf,3] i32); it parses the header instead of assuming it"""
    raw = open(path, "rb").read()
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    lines = raw[:end].decode("ascii").split("\n")
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0"
    elements, props = [], {}
    for ln in lines[2:]:
        w = ln.split()
        if w[:1] == ["element"]:
            elements.append((w[1], int(w[2])))
            props[w[1]] = []
        elif w[:1] == ["property"]:
            props[elements[-1][0]].append(w[1:])
    assert [e[0] for e in elements] == ["vertex", "face"]
    assert props["vertex"] == [["float", n] for n in ("x", "y", "z", "nx", "ny", "nz")]
    assert props["face"] == [["list", "uchar", "int", "vertex_indices"]]
    nv, nf = elements[0][1], elements[1][1]
    assert len(raw) == end + nv * 24 + nf * 13
    vert = np.frombuffer(raw, dtype="<f4", count=nv * 6, offset=end).reshape(nv, 6)
    face = np.frombuffer(raw, dtype=np.dtype([("n", "u1"), ("v", "<i4", (3,))]), count=nf, offset=end + nv * 24)
    assert (face["n"] == 3).all()
    return vert[:, :3].copy(), vert[:, 3:].copy(), face["v"].astype(np.int32).reshape(nf, 3)


def sphere_tsdf(n=24, centre=11.3, radius=8.0, band=3.0):
    """v = clamp((r - radius) / band, -1, 1) with the saturated far side written as 2 instead of 1: the value 1 is the reference's
    "unobserved" marker, which the field turns into +1 (inside) and which would wrap the sphere in a second, inverted surface;
    2 clips to the g = -1 that the clamp means"""
    i = np.indices((n, n, n)).astype(np.float64)
    r = np.sqrt(((i - centre) ** 2).sum(0))
    return tsdf_of_field(-np.clip((r - radius) / band, -1, 1).astype(F))


# smallest dot product between the oracle's normals and the analytic radial direction on sphere_tsdf() is 0.9999945 (measured on
# the CPU, tests/test_mesh_cpu.py); the threshold leaves 10 % of its distance from 1
SPHERE_MIN_DOT = 1.0 - 1.1 * (1.0 - 0.9999945)
