"""GPU: r2_isosurface_count / r2_isosurface_fill through mesh.isosurface against tests/isosurface_ref.py -- vertices and normals
bit for bit, faces as oriented sets -- at the shapes where the kernels take another path (csrc/isosurface.hip: 4096 points per
workgroup, 1024 per wave, 256 workgroup sums per thread of the scan); snapping onto the Gaussian field; the command line and
train.py --save_mesh."""
import os

import numpy as np
import pytest
import torch

from tests import isosurface_ref as R
from tests.test_isosurface_cpu import cell_pattern, read_ply, read_stl

pytestmark = pytest.mark.gpu


def run(gpu, vol, level, center=None, sVoxel=None, **kw):
    from r2_gaussian_amd.mesh import isosurface
    out = isosurface(torch.from_numpy(np.ascontiguousarray(vol, np.float32)).to(gpu), level, center, sVoxel, **kw)
    return [None if t is None else t.cpu().numpy() for t in out]


def frame(shape, center, sVoxel):
    from r2_gaussian_amd.mesh import _frame
    o, s = _frame(shape, center, sVoxel)
    return [np.float32(x) for x in o], [np.float32(x) for x in s]


def check(gpu, vol, level, center=None, sVoxel=None):
    """verts and normals bit-identical to the reference, faces equal as oriented sets, a second call identical."""
    v, f, n = run(gpu, vol, level, center, sVoxel)
    o, s = frame(vol.shape, center, sVoxel)
    rv, rf, rn = R.isosurface_ref(vol, level, o, s)
    assert v.dtype == np.float32 and f.dtype == np.int32 and n.dtype == np.float32
    assert v.shape == rv.shape and f.shape == rf.shape
    assert np.array_equal(v.view(np.uint32), rv.view(np.uint32)), "vertices differ in bits"
    assert np.array_equal(n.view(np.uint32), rn.view(np.uint32)), "normals differ in bits"
    assert np.array_equal(R.canonical_faces(f), R.canonical_faces(rf))
    v2, f2, n2 = run(gpu, vol, level, center, sVoxel)
    assert np.array_equal(v.view(np.uint32), v2.view(np.uint32)) and np.array_equal(n.view(np.uint32), n2.view(np.uint32))
    assert np.array_equal(f, f2)
    return v, f, n


def noise(shape, seed):
    return np.random.RandomState(seed).uniform(0.0, 1.0, shape).astype(np.float32)


def test_every_pattern_of_one_cell(gpu):
    rng = np.random.RandomState(11)
    for pattern in range(256):
        check(gpu, cell_pattern(pattern, rng), 0.0)


@pytest.mark.parametrize("shape", [(1, 5, 7), (4, 1, 3)])
def test_no_cells(gpu, shape):
    v, f, n = check(gpu, noise(shape, 1), 0.5)
    assert v.shape == (0, 3) and f.shape == (0, 3) and n.shape == (0, 3)


# (5, 9, 100): z rows straddle a wave's run of 1024 points and a workgroup's range of 4096
@pytest.mark.parametrize("shape", [(2, 2, 2), (3, 5, 67), (65, 2, 2), (2, 2, 129), (5, 9, 100)])
def test_edge_shapes(gpu, shape):
    v, f, _ = check(gpu, noise(shape, 2), 0.5, center=(0.1, -0.2, 0.3), sVoxel=(1.0, 1.5, 0.7))
    assert f.shape[0] > 0


def test_noise_17_19_23(gpu):
    check(gpu, noise((17, 19, 23), 3), 0.5)


def test_more_workgroups_than_scan_threads(gpu):
    """257 workgroups of 4096 points: a thread of the scan owns two workgroup sums.  A smooth field, so that the reference
    stays quick; its surface crosses every workgroup."""
    nx, ny, nz = 16, 16, 4100
    i, j, k = np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij")
    vol = (np.cos(0.37 * k) + 0.03 * i - 0.02 * j).astype(np.float32)
    assert -(-vol.size // 4096) == 257
    v, f, _ = check(gpu, vol, 0.25)
    assert f.shape[0] > 257


def test_level_outside_the_range_gives_nothing(gpu):
    vol = noise((6, 7, 8), 4)
    for level in (2.0, -1.0):
        v, f, n = check(gpu, vol, level)
        assert v.shape == (0, 3) and f.shape == (0, 3)


def test_values_equal_to_the_level(gpu):
    vol = np.pad(np.random.RandomState(5).randint(0, 3, (6, 5, 9)).astype(np.float32), 1)
    v, f, _ = check(gpu, vol, 1.0)
    assert f.shape[0] > 0 and R.is_closed_oriented(f)


def test_invalid_values_raise(gpu):
    vol = noise((5, 6, 7), 6)
    vol[2, 3, 4] = np.nan
    with pytest.raises(ValueError, match="1 invalid"):
        run(gpu, vol, 0.5)
    vol[0, 0, 0], vol[4, 5, 6] = np.inf, -3e38
    with pytest.raises(ValueError, match="3 invalid"):
        run(gpu, vol, 0.5)
    with pytest.raises(ValueError, match="fill"):
        run(gpu, noise((3, 3, 3), 0), 0.5, closed=True, fill=0.5)


def test_closed_and_normals_off(gpu):
    vol = noise((17, 19, 23), 3) * 0.8 + 0.2
    c, s = (0.0, 0.5, -0.5), (1.7, 1.9, 2.3)
    v, f, n = run(gpu, vol, 0.6, c, s)
    assert not R.is_closed_oriented(f)   # the surface reaches the border
    vc, fc, nc = run(gpu, vol, 0.6, c, s, closed=True)
    assert R.is_closed_oriented(fc) and R.signed_volume(vc, fc) > 0
    # the closed mesh is the padded volume's, one voxel further out
    from r2_gaussian_amd.mesh import _frame
    o, d = _frame(vol.shape, c, s)   # float64; the origin moves by one voxel before it is rounded
    rv, rf, rn = R.isosurface_ref(np.pad(vol, 1), 0.6, [np.float32(a - b) for a, b in zip(o, d)], [np.float32(b) for b in d])
    assert np.array_equal(vc.view(np.uint32), rv.view(np.uint32)) and np.array_equal(nc.view(np.uint32), rn.view(np.uint32))
    assert np.array_equal(R.canonical_faces(fc), R.canonical_faces(rf))
    v0, f0, n0 = run(gpu, vol, 0.6, c, s, normals=False)
    assert n0 is None and np.array_equal(v0.view(np.uint32), v.view(np.uint32)) and np.array_equal(f0, f)


def test_mesh_measures_on_the_device(gpu):
    from r2_gaussian_amd.mesh import isosurface, mesh_area, mesh_volume
    n = 17
    ax = np.linspace(-1.0, 1.0, n)
    x, y, z = np.meshgrid(ax, ax, ax, indexing="ij")
    vol = torch.from_numpy((0.7 - np.sqrt(x * x + y * y + z * z)).astype(np.float32)).to(gpu)
    v, f, _ = isosurface(vol, 0.0)
    a, w = mesh_area(v, f), mesh_volume(v, f)
    assert a.is_cuda and a.dtype == torch.float64 and w.is_cuda
    vn, fn = v.cpu().numpy(), f.cpu().numpy()
    assert abs(float(a) - R.area(vn, fn)) <= 1e-12 * R.area(vn, fn) and abs(float(w) - R.signed_volume(vn, fn)) <= 1e-10


def test_snap_to_field_reaches_the_models_level_set(gpu):
    """One isotropic Gaussian (rho 1, s 0.2) at the origin, level 0.3, 24^3 voxels over [-0.5, 0.5]^3: the level set is the sphere
    of radius s sqrt(2 ln(rho / level)).  Measured on the MI355X: see DESIGN.md section 4, "Isosurface extraction"."""
    from r2_gaussian_amd.field import query_points, voxel_centres
    from r2_gaussian_amd.mesh import isosurface, model_isosurface, snap_to_field
    level, s = 0.3, 0.2
    radius = s * np.sqrt(2.0 * np.log(1.0 / level))
    xyz = torch.zeros((1, 3), device=gpu)
    dens = torch.ones((1, 1), device=gpu)
    scal = torch.full((1, 3), s, device=gpu)
    rot = torch.tensor([[1.0, 0.0, 0.0, 0.0]], device=gpu)
    c, n, sv = (0.0, 0.0, 0.0), (24, 24, 24), (1.0, 1.0, 1.0)
    vol = query_points(voxel_centres(c, n, sv, gpu), xyz, dens, scal, rot)
    v0, f0, _ = isosurface(vol, level, c, sv)
    assert v0.shape[0] > 100 and R.is_closed_oriented(f0.cpu().numpy())
    v1, n1 = snap_to_field(v0, level, xyz, dens, scal, rot, max_step=0.5 / 24)
    r0 = v0.to(torch.float64).norm(dim=1)
    r1 = v1.to(torch.float64).norm(dim=1)
    e0, e1 = float((r0 - radius).abs().max()), float((r1 - radius).abs().max())
    en = float((n1.to(torch.float64) - v1.to(torch.float64) / r1[:, None]).norm(dim=1).max())
    print("radial error: grid mesh %.3e, snapped %.3e; snapped normals against the radial direction %.3e" % (e0, e1, en))
    assert e1 <= 1e-5
    assert e1 * 100.0 <= e0
    assert en <= 1e-5
    # model_isosurface is the same chain; closed, the sphere (which does not reach the border) is the same surface
    vm, fm, nm = model_isosurface(xyz, dens, scal, rot, level, c, n, sv, closed=False)
    assert torch.equal(vm, v1) and torch.equal(fm, f0) and torch.equal(nm, n1)
    vc, fc, _ = model_isosurface(xyz, dens, scal, rot, level, c, n, sv)
    assert fc.shape == f0.shape and float((vc.to(torch.float64).norm(dim=1) - radius).abs().max()) <= 1e-5
    # a vertex where the gradient vanishes stays where it is
    far = torch.tensor([[50.0, 0.0, 0.0]], device=gpu)
    vf, nf = snap_to_field(far, level, xyz, dens, scal, rot)
    assert torch.equal(vf, far) and float(nf.abs().max()) == 0.0


def _blob(n, c0, sigma, rho):
    ax = -1 + (np.arange(n) + 0.5) * 2.0 / n
    X, Y, Z = np.meshgrid(ax, ax, ax, indexing="ij")
    return (rho * np.exp(-((X - c0[0]) ** 2 + (Y - c0[1]) ** 2 + (Z - c0[2]) ** 2) / (2 * sigma ** 2))).astype(np.float32)


def test_save_mesh_and_the_command_line(gpu, tmp_path, capsys):
    """train.py --save_mesh on a tiny case written by datagen, then python -m r2_gaussian_amd.mesh on its model and on its
    volume (both mains in this process): the files exist and parse."""
    from r2_gaussian_amd import datagen as D
    from r2_gaussian_amd import mesh as MS
    from r2_gaussian_amd import scene as S
    from r2_gaussian_amd import train as TR
    n, iters = 32, 20
    vol = _blob(n, (0.1, -0.2, 0.05), 0.3, 0.6) + _blob(n, (-0.3, 0.25, -0.1), 0.15, 0.5)
    cfg = dict(S.CONE_BEAM, nVoxel=[n, n, n], nDetector=[64, 64], noise=False, totalAngle=360.0, startAngle=0.0)
    case = D.generate(vol, cfg, str(tmp_path / "data"), "phantom", n_train=12, n_test=2, seed=0)
    out = str(tmp_path / "out")
    TR.main(["-s", case, "-m", out, "--iterations", str(iters), "--test_iterations", str(iters), "--quiet", "--save_mesh", "0.2"])
    pc = os.path.join(out, "point_cloud", "iteration_%d" % iters)
    pv, pf, props = read_ply(os.path.join(pc, "mesh.ply"))
    assert props == ["x", "y", "z", "nx", "ny", "nz"] and pv.shape[0] > 0 and pf.shape[0] > 0
    assert pf.min() >= 0 and pf.max() < pv.shape[0] and np.isfinite(pv).all()
    assert R.is_closed_oriented(pf)   # model_isosurface closes the surface
    meta = os.path.join(case, "meta_data.json")
    MS.main(["--model", os.path.join(pc, "point_cloud.pickle"), "--meta", meta, "--level", "0.2", "--snap", "--closed",
             "--out", str(tmp_path / "model.ply")])
    mv, mf, _ = read_ply(str(tmp_path / "model.ply"))
    # what --save_mesh wrote, up to the rounding of the activations (the trainer's fused kernel against model_io's torch)
    assert R.is_closed_oriented(mf) and abs(R.area(mv[:, :3], mf) - R.area(pv[:, :3], pf)) <= 1e-2 * R.area(pv[:, :3], pf)
    MS.main(["--volume", os.path.join(pc, "vol_pred.npy"), "--meta", meta, "--level", "0.2", "--out", str(tmp_path / "vol.stl")])
    sn, sv = read_stl(str(tmp_path / "vol.stl"))
    assert sv.shape[0] > 0 and np.isfinite(sv).all() and np.isfinite(sn).all()
    assert "triangles" in capsys.readouterr().out
