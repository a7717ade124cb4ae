"""numpy float32 restatement of r2_isosurface_count / r2_isosurface_fill (include/r2hip.h, csrc/isosurface.hip), operation for
operation: marching tetrahedra on the Kuhn subdivision of the voxel lattice.  numpy's float32 array operations round every
operation separately, as the kernels do (they are compiled without FMA contraction), so vertices and normals are compared bit
for bit.  The face ORDER is the implementation's own; compare faces by ``canonical_faces``.

Also here: the mesh checks the tests share (closedness, Euler characteristic, area, volume), in float64."""
import itertools

import numpy as np

F = np.float32
INVALID_ABOVE = F(1e38)

PERMS = list(itertools.permutations(range(3)))   # (a, b, c): 000 -> +e_a -> +e_a+e_b -> 111, in the kernel's order
MIRRORED = [False, True, True, False, False, True]   # odd permutations: negatively oriented corners

# The triangles of a tetrahedron with positively oriented corners 0..3, by its sign case (bit v: corner v inside), as pairs of
# corners (the edge a triangle's vertex lies on).  For one inside corner s and an even permutation (s, x, y, z) of the corners
# the triangle (sx, sy, sz) is counter-clockwise seen from outside; three inside: reversed.  For two inside corners and an even
# permutation (s1, s2, o1, o2) the quad is (s1o1, s1o2, s2o2, s2o1), split along its first and third corner.
TET_TRIANGLES = {
    0: [],
    1: [((0, 1), (0, 2), (0, 3))],
    2: [((0, 1), (1, 3), (1, 2))],
    3: [((0, 2), (0, 3), (1, 3)), ((0, 2), (1, 3), (1, 2))],
    4: [((0, 2), (1, 2), (2, 3))],
    5: [((0, 3), (0, 1), (1, 2)), ((0, 3), (1, 2), (2, 3))],
    6: [((0, 1), (1, 3), (2, 3)), ((0, 1), (2, 3), (0, 2))],
    7: [((0, 3), (1, 3), (2, 3))],
    8: [((0, 3), (2, 3), (1, 3))],
    9: [((0, 1), (0, 2), (2, 3)), ((0, 1), (2, 3), (1, 3))],
    10: [((1, 2), (0, 1), (0, 3)), ((1, 2), (0, 3), (2, 3))],
    11: [((0, 2), (2, 3), (1, 2))],
    12: [((0, 2), (1, 2), (1, 3)), ((0, 2), (1, 3), (0, 3))],
    13: [((0, 1), (1, 2), (1, 3))],
    14: [((0, 1), (0, 3), (0, 2))],
    15: [],
}


def tet_corners(t):
    """Corner ids (dx + 2 dy + 4 dz) of tetrahedron t of a cell."""
    a, b, _ = PERMS[t]
    return [0, 1 << a, (1 << a) | (1 << b), 7]


def _delta(c):
    return c & 1, (c >> 1) & 1, (c >> 2) & 1


def invalid_count(vol):
    v = np.asarray(vol, F)
    with np.errstate(invalid="ignore"):
        return int((~(np.abs(v) <= INVALID_ABOVE)).sum())


def lattice_gradient(vol, spacing):
    """[nx,ny,nz,3] float32: central differences / (2 s), one-sided / s on a border (every dimension >= 2)."""
    vol = np.asarray(vol, F)
    g = np.zeros(vol.shape + (3,), F)
    for a in range(3):
        s = F(spacing[a])
        f = np.moveaxis(vol, a, 0)
        out = np.moveaxis(g[..., a], a, 0)
        out[1:-1] = (f[2:] - f[:-2]) / (F(2.0) * s)
        out[0] = (f[1] - f[0]) / s
        out[-1] = (f[-1] - f[-2]) / s
    return g


def isosurface_ref(vol, level, origin=(0.0, 0.0, 0.0), spacing=(1.0, 1.0, 1.0), normals=True):
    """-> (verts [Nv,3] f32, faces [Nf,3] int32, normals [Nv,3] f32 or None)."""
    vol = np.ascontiguousarray(vol, F)
    nx, ny, nz = vol.shape
    level = F(level)
    o = [F(v) for v in origin]
    s = [F(v) for v in spacing]
    empty = (np.zeros((0, 3), F), np.zeros((0, 3), np.int32), np.zeros((0, 3), F) if normals else None)
    if min(nx, ny, nz) < 2:
        return empty
    with np.errstate(invalid="ignore"):
        inside = vol >= level
    N = nx * ny * nz
    # crossed[L, c - 1]: the edge of direction code c owned by point L exists and is crossed
    crossed = np.zeros((nx, ny, nz, 7), bool)
    for c in range(1, 8):
        dx, dy, dz = _delta(c)
        crossed[:nx - dx, :ny - dy, :nz - dz, c - 1] = inside[:nx - dx, :ny - dy, :nz - dz] != inside[dx:, dy:, dz:]
    crossed = crossed.reshape(N, 7)
    owner, bit = np.nonzero(crossed)          # row-major: by (linear index, code) ascending
    nv = owner.shape[0]
    vid = np.full((N, 7), -1, np.int64)
    vid[owner, bit] = np.arange(nv)
    d = np.stack([(bit + 1) & 1, ((bit + 1) >> 1) & 1, (bit + 1) >> 2], 1)
    pi, pj, pk = np.unravel_index(owner, (nx, ny, nz))
    p = np.stack([pi, pj, pk], 1)
    q = p + d
    fa = vol[p[:, 0], p[:, 1], p[:, 2]]
    fb = vol[q[:, 0], q[:, 1], q[:, 2]]
    with np.errstate(all="ignore"):
        t = (level - fa) / (fb - fa)
        verts = np.empty((nv, 3), F)
        for a in range(3):
            pa = np.where(d[:, a] == 1, p[:, a].astype(F) + t, p[:, a].astype(F)).astype(F)
            verts[:, a] = o[a] + pa * s[a]
        nrm = None
        if normals:
            g = lattice_gradient(vol, s)
            ga = g[p[:, 0], p[:, 1], p[:, 2]]
            gb = g[q[:, 0], q[:, 1], q[:, 2]]
            ge = (ga + t[:, None] * (gb - ga)).astype(F)
            n = np.sqrt((ge[:, 0] * ge[:, 0] + ge[:, 1] * ge[:, 1]) + ge[:, 2] * ge[:, 2])
            ok = n > 0
            nrm = np.zeros((nv, 3), F)
            nrm[ok] = (-ge[ok]) / n[ok, None]
    # faces
    L = np.arange(N, dtype=np.int64).reshape(nx, ny, nz)
    cellL = L[:-1, :-1, :-1].reshape(-1)
    cin = [inside[dx:nx - 1 + dx, dy:ny - 1 + dy, dz:nz - 1 + dz].reshape(-1) for dx, dy, dz in map(_delta, range(8))]
    cL = [cellL + (dx * ny + dy) * nz + dz for dx, dy, dz in map(_delta, range(8))]
    parts = []
    for tet in range(6):
        cs = tet_corners(tet)
        case = sum(cin[cs[v]].astype(np.int64) << v for v in range(4))
        for m in range(1, 15):
            sel = np.nonzero(case == m)[0]
            if sel.size == 0:
                continue
            for r, tri in enumerate(TET_TRIANGLES[m]):
                ids = [vid[cL[cs[a]][sel], cs[b] - cs[a] - 1] for a, b in tri]
                if MIRRORED[tet]:
                    ids = [ids[0], ids[2], ids[1]]
                key = (cellL[sel] * 6 + tet) * 2 + r
                parts.append((key, np.stack(ids, 1)))
    if parts:
        key = np.concatenate([k for k, _ in parts])
        faces = np.concatenate([f for _, f in parts])[np.argsort(key, kind="stable")]
        assert (faces >= 0).all()
        faces = faces.astype(np.int32)
    else:
        faces = np.zeros((0, 3), np.int32)
    return verts, faces, nrm


def canonical_faces(faces):
    """Every row rotated to start at its smallest index, rows sorted: equal for two meshes with the same oriented faces."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    if f.shape[0] == 0:
        return f
    r = np.argmin(f, 1)
    f = np.stack([np.take_along_axis(f, ((r + k) % 3)[:, None], 1)[:, 0] for k in range(3)], 1)
    return f[np.lexsort((f[:, 2], f[:, 1], f[:, 0]))]


def directed_edges(faces):
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    return np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])


def is_closed_oriented(faces):
    """Every directed edge occurs once and its reverse once (degenerate faces, whose vertices may coincide in SPACE, have
    distinct ids and take part like any other)."""
    e = directed_edges(faces)
    if e.shape[0] == 0:
        return True
    big = int(e.max()) + 1
    k = e[:, 0] * big + e[:, 1]
    kr = e[:, 1] * big + e[:, 0]
    u, n = np.unique(k, return_counts=True)
    return bool((n == 1).all() and np.array_equal(u, np.unique(kr)))


def euler_characteristic(nverts, faces):
    e = directed_edges(faces)
    und = np.unique(np.sort(e, 1), axis=0)
    return int(nverts) - und.shape[0] + np.asarray(faces).reshape(-1, 3).shape[0]


def area(verts, faces):
    v = np.asarray(verts, np.float64)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    return float(0.5 * np.linalg.norm(np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]]), axis=1).sum())


def signed_volume(verts, faces):
    v = np.asarray(verts, np.float64)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    return float((np.einsum("ij,ij->i", v[f[:, 0]], np.cross(v[f[:, 1]], v[f[:, 2]]))).sum() / 6.0)
