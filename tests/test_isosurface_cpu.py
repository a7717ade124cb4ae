"""CPU: pins tests/isosurface_ref.py, the numpy float32 restatement of the isosurface kernels (include/r2hip.h,
r2_isosurface_count), on surfaces whose topology, area and volume are known, on all 256 inside / outside patterns of one cell,
and the mesh writers and measures of r2_gaussian_amd/mesh.py (host code)."""
import struct

import numpy as np
import pytest
import torch

from tests import isosurface_ref as R


def sphere(n):
    ax = np.linspace(-1.0, 1.0, n)
    x, y, z = np.meshgrid(ax, ax, ax, indexing="ij")
    return (0.7 - np.sqrt(x * x + y * y + z * z)).astype(np.float32), 2.0 / (n - 1)


@pytest.fixture(scope="module")
def spheres():
    out = {}
    for n in (9, 17):
        vol, h = sphere(n)
        out[n] = R.isosurface_ref(vol, 0.0, (-1.0, -1.0, -1.0), (h, h, h))
    return out


@pytest.mark.parametrize("n,nv,nf", [(9, 386, 768), (17, 1730, 3456)])
def test_sphere_is_closed_oriented_and_a_sphere(spheres, n, nv, nf):
    v, f, nrm = spheres[n]
    assert v.dtype == np.float32 and f.dtype == np.int32 and nrm.dtype == np.float32
    assert (v.shape[0], f.shape[0]) == (nv, nf)
    assert R.is_closed_oriented(f)
    assert R.euler_characteristic(v.shape[0], f) == 2
    assert R.signed_volume(v, f) > 0
    # the normals are the outward radial direction, up to the lattice differences' error
    radial = v / np.linalg.norm(v, axis=1, keepdims=True)
    assert ((nrm * radial).sum(1) > 0.9).all()


def test_sphere_volume_converges_at_second_order(spheres):
    exact = 4.0 / 3.0 * np.pi * 0.7 ** 3
    e9, e17 = (abs(R.signed_volume(*spheres[n][:2]) - exact) for n in (9, 17))
    print("sphere volume error: n = 9: %.5f, n = 17: %.5f, ratio %.2f" % (e9, e17, e9 / e17))
    assert e9 >= 3.0 * e17


def test_torus_has_genus_one():
    n = 15
    ax = np.linspace(-1.0, 1.0, n)
    x, y, z = np.meshgrid(ax, ax, ax, indexing="ij")
    vol = (0.22 - np.sqrt((np.sqrt(x * x + y * y) - 0.55) ** 2 + z * z)).astype(np.float32)
    v, f, _ = R.isosurface_ref(vol, 0.0)
    assert f.shape[0] > 0 and R.is_closed_oriented(f)
    assert R.euler_characteristic(v.shape[0], f) == 0
    assert R.signed_volume(v, f) > 0


def test_padded_noise_is_closed_and_oriented():
    rng = np.random.RandomState(3)
    vol = np.pad(rng.uniform(0.2, 1.0, (5, 6, 7)).astype(np.float32), 1)
    v, f, nrm = R.isosurface_ref(vol, 0.6)
    assert f.shape[0] > 0 and R.is_closed_oriented(f)
    assert R.signed_volume(v, f) > 0
    assert np.isfinite(nrm).all()


def test_plane():
    from r2_gaussian_amd.mesh import mesh_area
    vol = np.broadcast_to(np.arange(6, dtype=np.float32)[:, None, None], (6, 4, 5)).copy()
    v, f, nrm = R.isosurface_ref(vol, 2.5)
    assert (v[:, 0] == 2.5).all()
    assert float(mesh_area(torch.from_numpy(v), torch.from_numpy(f))) == 12.0
    assert R.area(v, f) == 12.0
    assert (nrm == np.array([-1.0, 0.0, 0.0], np.float32)).all()
    # the inside is x >= 2.5: the geometric normals point to -x as well
    g = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    assert (g[:, 0] < 0).all() and (g[:, 1:] == 0).all()


def cell_pattern(pattern, rng):
    """One 2 x 2 x 2 cell: corner dx + 2 dy + 4 dz inside (> 0) iff its bit of ``pattern`` is set, with random magnitudes."""
    mag = rng.uniform(0.1, 1.0, 8).astype(np.float32)
    vol = np.empty((2, 2, 2), np.float32)
    for c in range(8):
        vol[c & 1, (c >> 1) & 1, c >> 2] = mag[c] if (pattern >> c) & 1 else -mag[c]
    return vol


def test_every_pattern_of_one_cell():
    rng = np.random.RandomState(11)
    corner = np.array([[c & 1, (c >> 1) & 1, c >> 2] for c in range(8)], np.float64)
    edges = [(u, v) for u in range(8) for v in range(8) if u != v and (u & v) == u]   # u's offsets are a subset of v's
    assert len(edges) == 19
    for pattern in range(256):
        vol = cell_pattern(pattern, rng)
        v, f, _ = R.isosurface_ref(vol, 0.0)
        ins = [(pattern >> c) & 1 for c in range(8)]
        assert v.shape[0] == sum(ins[u] != ins[w] for u, w in edges), pattern
        # the faces come tetrahedron by tetrahedron; each one's geometric normal points from its inside corners to its
        # outside corners
        at = 0
        for tet in range(6):
            cs = R.tet_corners(tet)
            k = sum(ins[c] for c in cs)
            n = 0 if k in (0, 4) else (2 if k == 2 else 1)
            if n:
                inside_c = np.mean([corner[c] for c in cs if ins[c]], 0)
                outside_c = np.mean([corner[c] for c in cs if not ins[c]], 0)
            for tri in f[at:at + n]:
                p = v[tri].astype(np.float64)
                g = np.cross(p[1] - p[0], p[2] - p[0])
                assert g @ (outside_c - inside_c) > 0, (pattern, tet)
            at += n
        assert at == f.shape[0], pattern


def test_degenerate_values_keep_the_surface_closed():
    rng = np.random.RandomState(5)
    vol = np.pad(rng.randint(0, 3, (4, 5, 3)).astype(np.float32), 1)
    v, f, _ = R.isosurface_ref(vol, 1.0)   # many corner values equal the level
    assert f.shape[0] > 0 and R.is_closed_oriented(f)


def test_no_cells_and_invalid_values():
    for shape in ((1, 5, 7), (4, 1, 3)):
        v, f, nrm = R.isosurface_ref(np.random.RandomState(0).rand(*shape).astype(np.float32), 0.5)
        assert v.shape == (0, 3) and f.shape == (0, 3) and nrm.shape == (0, 3)
    vol = np.zeros((2, 3, 4), np.float32)
    vol[0, 0, 0], vol[1, 1, 1], vol[1, 2, 3], vol[0, 1, 0] = np.nan, np.inf, -2e38, 1e38
    assert R.invalid_count(vol) == 3


def read_ply(path):
    with open(path, "rb") as fh:
        data = fh.read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    head = data[:end].decode("ascii").split("\n")
    assert head[0] == "ply" and head[1] == "format binary_little_endian 1.0"
    nv = [int(l.split()[2]) for l in head if l.startswith("element vertex")][0]
    nf = [int(l.split()[2]) for l in head if l.startswith("element face")][0]
    props = [l.split()[2] for l in head if l.startswith("property float")]
    v = np.frombuffer(data, "<f4", nv * len(props), end).reshape(nv, len(props))
    at = end + v.nbytes
    faces = []
    for _ in range(nf):
        k, a, b, c = struct.unpack_from("<Biii", data, at)
        assert k == 3
        faces.append((a, b, c))
        at += 13
    assert at == len(data)
    return v, np.array(faces, np.int32).reshape(-1, 3), props


def read_stl(path):
    with open(path, "rb") as fh:
        data = fh.read()
    n, = struct.unpack_from("<I", data, 80)
    assert len(data) == 84 + 50 * n
    rec = np.frombuffer(data, np.dtype([("n", "<f4", (3,)), ("v", "<f4", (3, 3)), ("a", "<u2")]), n, 84)
    return rec["n"], rec["v"]


def test_writers_round_trip(spheres, tmp_path):
    from r2_gaussian_amd.mesh import write_ply, write_stl
    v, f, nrm = spheres[9]
    tv, tf, tn = torch.from_numpy(v), torch.from_numpy(f), torch.from_numpy(nrm)
    write_ply(str(tmp_path / "a.ply"), tv, tf, tn)
    pv, pf, props = read_ply(str(tmp_path / "a.ply"))
    assert props == ["x", "y", "z", "nx", "ny", "nz"]
    assert np.array_equal(pv[:, :3], v) and np.array_equal(pv[:, 3:], nrm) and np.array_equal(pf, f)
    write_ply(str(tmp_path / "b.ply"), tv, tf)
    pv, pf, props = read_ply(str(tmp_path / "b.ply"))
    assert props == ["x", "y", "z"] and np.array_equal(pv, v) and np.array_equal(pf, f)
    write_stl(str(tmp_path / "a.stl"), tv, tf)
    sn, sv = read_stl(str(tmp_path / "a.stl"))
    assert np.array_equal(sv, v[f])
    g = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]]).astype(np.float64)
    assert np.allclose(sn, g / np.linalg.norm(g, axis=1, keepdims=True), atol=1e-6)


def test_mesh_measures_match_the_reference_checks(spheres):
    from r2_gaussian_amd.mesh import mesh_area, mesh_volume
    v, f, _ = spheres[17]
    tv, tf = torch.from_numpy(v), torch.from_numpy(f)
    assert mesh_area(tv, tf).dtype == torch.float64
    assert abs(float(mesh_area(tv, tf)) - R.area(v, f)) <= 1e-12 * R.area(v, f)
    assert abs(float(mesh_volume(tv, tf)) - R.signed_volume(v, f)) <= 1e-12
    assert abs(float(mesh_area(tv, tf)) - 4 * np.pi * 0.49) < 0.05 * 4 * np.pi * 0.49


def test_cpu_volumes_are_refused():
    from r2_gaussian_amd import _lib
    from r2_gaussian_amd.mesh import isosurface, snap_to_field
    with pytest.raises(_lib.R2HipError):
        isosurface(torch.zeros(3, 3, 3), 0.5)
    with pytest.raises(_lib.R2HipError):
        snap_to_field(torch.zeros(4, 3), 0.5, torch.zeros(1, 3), torch.ones(1, 1), torch.ones(1, 3), torch.ones(1, 4))
