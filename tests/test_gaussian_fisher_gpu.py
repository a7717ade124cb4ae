"""GPU: the Fisher diagonal and the two predictive variances (r2_gaussian_amd.uncertainty; csrc/gaussian_fisher.hip,
csrc/gaussian_variance.hip) against the float64 restatement of their contract (tests/gaussian_fisher_ref.py).

Bracket: every quantity is a sum of addends >= 0 and the contract lets a pair with q > 32 be summed or skipped, so the kernels
must lie between the float64 sum over the pairs with q <= 32 and the float64 sum over every pair.  Each limit is widened by
4 x e32 x (F64 + 2^-40 N) of that limit plus the float32 underflow floor of gaussian_project_ref: e32 is the measured error of
the float32 restatement for that scene, quantity and group (tests/golden/gaussian_fisher/e32.json; the CPU test holds every one
below 0.1), N the sum with every per-pair derivative replaced by its magnitude, and the factor 4 covers the device's expf /
sqrt against numpy's and the different association of the sums.  No component, pixel or point is excluded.
"""
import os

import numpy as np
import pytest
import torch

from tests import gaussian_field_ref as RF
from tests import gaussian_fisher_ref as R

pytestmark = pytest.mark.gpu

E32 = R.load_e32()
GUARD = 16          # guard words on either side of every buffer the C ABI writes
SENTINEL = -7.25


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _cloud(cloud, dev):
    return [_t(a, dev) for a in cloud]


def _var(var, dev):
    return tuple(_t(var[k], dev) for k in R.GROUPS)


def _fisher(sc, dev, weights=None, views=None, cloud=None):
    from r2_gaussian_amd.uncertainty import fisher_diagonal
    return fisher_diagonal(sc["views"] if views is None else views, *_cloud(sc["cloud"] if cloud is None else cloud, dev),
                           weights=None if weights is None else _t(weights, dev), scale_modifier=sc["mod"])


def _pvar(sc, var, dev):
    from r2_gaussian_amd.uncertainty import projection_variance
    return projection_variance(sc["views"], *_cloud(sc["cloud"], dev), _var(var, dev), scale_modifier=sc["mod"])


def _fvar(sc, var, dev, sort=False, points=None, cloud=None):
    from r2_gaussian_amd.uncertainty import field_variance
    return field_variance(_t(sc["points"] if points is None else points, dev), *_cloud(sc["cloud"] if cloud is None else cloud, dev),
                          _var(var, dev), scale_modifier=sc["mod"], sort=sort)


def _rows(F):
    """CloudTuple -> [11, P] float64 on the host."""
    return np.concatenate([f.cpu().numpy().astype(np.float64).reshape(f.shape[0], -1).T for f in F], 0)


# ------------------------------------------------------------------------------------------------------ against float64
@pytest.mark.parametrize("name", R.PROJ_SCENES)
def test_fisher_diagonal_vs_float64(gpu, name):
    """Entry 1 on every scene of gaussian_project_ref (P = 1 on 8 x 8, 300 Gaussians on one tile, a Gaussian covering the
    detector, off the detector, behind and containing the source, raw quaternion norms, scale_modifier 0.5, sigma 0.01 from six
    units away), the 260 x 264 detector of gaussian_project_rays_ref in cone beam, and an all-isotropic copy of cone_p7, with
    weights in [0.5, 1.5): all eleven components of every Gaussian inside the bracket."""
    r = R.projector_reference(name)
    sc = r["scene"]
    F = _fisher(sc, gpu, r["weights"])
    P = sc["cloud"][0].shape[0]
    assert [tuple(f.shape) for f in F] == [(P, 3), (P, 1), (P, 3), (P, 4)] and all(f.dtype == torch.float32 for f in F)
    got = _rows(F)
    for k in R.GROUPS:
        s = R.ROWS[k]
        R.bracket(got[s], [r["F"][0][s], r["F"][1][s]], [r["NF"][0][s], r["NF"][1][s]], E32["fisher"][name][k], "%s fisher %s" % (name, k))


@pytest.mark.parametrize("name", R.PROJ_SCENES)
def test_projection_variance_vs_float64(gpu, name):
    """Entry 3 on the same scenes, pixel by pixel."""
    r = R.projector_reference(name)
    sc = r["scene"]
    out = _pvar(sc, r["var"], gpu)
    assert out.shape == (len(sc["views"]), sc["H"], sc["W"]) and out.dtype == torch.float32
    R.bracket(out.cpu().numpy(), r["pv"], r["Npv"], E32["projection_variance"][name], name + " projection variance")


@pytest.mark.parametrize("name", R.FIELD_SCENES)
def test_field_variance_vs_float64(gpu, name):
    """Entry 2 on every scene of gaussian_field_ref: an oblique plane, a 12^3 patch, scattered points, the block tails N = 1,
    255, 256, 257, 513, P = 700 (two full rounds of 256 and a partial one), P = 0, points outside every sphere, cloud and points
    100 extents away, sigma = 5e-4, non-finite rows and points, raw quaternions, scale_modifier 0.5 and 2."""
    r = R.field_reference(name)
    sc = r["scene"]
    out = _fvar(sc, r["var"], gpu)
    assert out.shape == sc["points"].shape[:-1] and out.dtype == torch.float32
    R.bracket(out.cpu().numpy(), r["pv"], r["Npv"], E32["field_variance"][name], name + " field variance")


@pytest.mark.parametrize("name", R.IDENTITY_SCENES)
def test_identity_between_fisher_and_projection_variance(gpu, name):
    """sum_pixels w * projection_variance = sum_it F_it v_it: the same set of pairs added in two orders by two kernels, both
    reduced in float64 on the host.  Tolerance: 4 x (e32 of entry 1 (its worst group) + e32 of entry 3) of the scene x the
    total's normaliser T64 + 2^-40 NT."""
    r = R.projector_reference(name)
    sc = r["scene"]
    a = float((_rows(_fisher(sc, gpu, r["weights"])) * R.stack(r["var"], np.float64)).sum())
    b = float((r["weights"].astype(np.float64) * _pvar(sc, r["var"], gpu).cpu().numpy().astype(np.float64)).sum())
    e = max(E32["fisher"][name].values()) + E32["projection_variance"][name]
    tol = 4.0 * e * R.normaliser(r["T"][1], r["NT"][1])
    print("%s identity: sum F v %.9e, sum w pvar %.9e, difference %.3e, tolerance %.3e, float64 %.9e" % (name, a, b, abs(a - b), tol, r["T"][1]))
    assert a > 0 and abs(a - b) <= tol


# ------------------------------------------------------------------------------------------------------ bit identities
def test_calls_are_reproducible(gpu):
    r = R.projector_reference("cone_p7")
    sc = r["scene"]
    assert all(torch.equal(a, b) for a, b in zip(_fisher(sc, gpu, r["weights"]), _fisher(sc, gpu, r["weights"])))
    assert torch.equal(_pvar(sc, r["var"], gpu), _pvar(sc, r["var"], gpu))
    f = R.field_reference("plane")
    assert torch.equal(_fvar(f["scene"], f["var"], gpu), _fvar(f["scene"], f["var"], gpu))


def test_no_weights_are_unit_weights(gpu):
    sc = R.proj_scene("cone_p7")
    ones = np.ones((len(sc["views"]), sc["H"], sc["W"]), np.float32)
    assert all(torch.equal(a, b) for a, b in zip(_fisher(sc, gpu), _fisher(sc, gpu, ones)))


def test_a_view_of_zero_weight_changes_no_bit(gpu):
    r = R.projector_reference("cone_p7")
    sc = r["scene"]
    extra = R.candidate_views("cone_p7", (1.2,))
    w = np.concatenate([r["weights"], np.zeros((1, sc["H"], sc["W"]), np.float32)], 0)
    assert all(torch.equal(a, b) for a, b in zip(_fisher(sc, gpu, r["weights"]), _fisher(sc, gpu, w, views=sc["views"] + extra)))


def test_doubling_the_densities(gpu):
    """Every derivative but d / d rho is linear in rho, and a factor 2 is exact in float32: F.density keeps its bits and the
    other ten components are multiplied by exactly 4."""
    r = R.projector_reference("cone_p7")
    sc = r["scene"]
    xyz, dens, scal, rot = sc["cloud"]
    F1, F2 = _fisher(sc, gpu, r["weights"]), _fisher(sc, gpu, r["weights"], cloud=(xyz, 2.0 * dens, scal, rot))
    assert torch.equal(F1.density, F2.density) and (F1.density > 0).all()
    for k in ("xyz", "scaling", "rotation"):
        assert torch.equal(4.0 * getattr(F1, k), getattr(F2, k)), k


@pytest.mark.parametrize("name", ["scattered", "tail_513"])
def test_field_variance_does_not_depend_on_the_order_of_the_points(gpu, name):
    """Permuting the points permutes the values bit for bit, and sort=True equals sort=False."""
    r = R.field_reference(name)
    sc = r["scene"]
    pts = sc["points"].reshape(-1, 3)
    perm = np.random.RandomState(9).permutation(pts.shape[0])
    out = _fvar(sc, r["var"], gpu).reshape(-1)
    assert (out > 0).any()
    assert torch.equal(_fvar(sc, r["var"], gpu, points=pts[perm]), out[_t(perm, gpu)])
    assert torch.equal(_fvar(sc, r["var"], gpu, sort=True).reshape(-1), out)


# ------------------------------------------------------------------------------------------------------ exact zeros
@pytest.mark.parametrize("name", ["cone_offdet", "parallel_offdet", "cone_behind"])
def test_untouched_gaussians_get_exact_zeros(gpu, name):
    """A Gaussian that projects off the detector, or lies behind the cone source: its Fisher row is exact zeros, the others'
    rows and the projection variance are bit-identical to the call without it."""
    r = R.projector_reference(name)
    sc = r["scene"]
    F = _fisher(sc, gpu, r["weights"])
    P = sc["cloud"][0].shape[0]
    keep = [i for i in range(P) if i not in sc["zero"]]
    F2 = _fisher(sc, gpu, r["weights"], cloud=tuple(a[keep] for a in sc["cloud"]))
    for a, b in zip(F, F2):
        assert (a[sc["zero"]] == 0).all() and torch.isfinite(a).all() and torch.equal(a[keep], b)
    without = dict(sc, cloud=tuple(a[keep] for a in sc["cloud"]))
    assert torch.equal(_pvar(sc, r["var"], gpu), _pvar(without, {k: v[keep] for k, v in r["var"].items()}, gpu))


def test_degenerate_gaussians_get_exact_zeros(gpu):
    """A scale of 0, a negative scale and a NaN mean (gauss_radius < 0): exact zero rows, and the rest untouched."""
    r = R.projector_reference("cone_p7")
    sc = r["scene"]
    xyz, dens, scal, rot = (a.copy() for a in sc["cloud"])
    scal[1, 0], scal[2, 1], xyz[3, 2] = 0.0, -0.1, np.nan
    F, F0 = _fisher(sc, gpu, r["weights"], cloud=(xyz, dens, scal, rot)), _fisher(sc, gpu, r["weights"])
    for a, b in zip(F, F0):
        assert (a[[1, 2, 3]] == 0).all() and torch.equal(a[[0, 4, 5, 6]], b[[0, 4, 5, 6]])


@pytest.mark.parametrize("name", ["far", "none", "bad"])
def test_field_variance_exact_zeros(gpu, name):
    """Points outside every sphere and P = 0: zeros.  `bad`: the NaN and inf points get 0, everything is finite, and the values
    are bit-identical to the query without the Gaussians with a NaN mean, an inf scale and a zero scale."""
    r = R.field_reference(name)
    sc = r["scene"]
    out = _fvar(sc, r["var"], gpu)
    if name in ("far", "none"):
        assert (out == 0).all()
        return
    zg, zp = sc["zero_gaussians"], sc["zero_points"]
    assert torch.isfinite(out).all() and (out[zp] == 0).all() and (out > 0).any()
    keep = [i for i in range(sc["cloud"][0].shape[0]) if i not in zg]
    out2 = _fvar(sc, {k: v[keep] for k, v in r["var"].items()}, gpu, cloud=tuple(a[keep] for a in sc["cloud"]))
    assert torch.equal(out, out2)


# ------------------------------------------------------------------------------------------------------ the C ABI itself
def _guarded(n, dev):
    whole = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.float32, device=dev)
    return whole, whole[GUARD:GUARD + n]


def _intact(whole, n):
    return bool((whole[:GUARD] == SENTINEL).all()) and bool((whole[GUARD + n:] == SENTINEL).all())


def test_c_abi_of_the_fisher_entry(gpu):
    """Through ctypes: guard words around the four outputs survive and the public layer returns the C entry's bits; invalid
    arguments return R2_ERR_INVALID and write nothing; P = 0 returns 0 and writes nothing."""
    from r2_gaussian_amd import _lib
    L = _lib.lib()
    r = R.projector_reference("cone_p300_small")
    sc = r["scene"]
    x, d, s, q = _cloud(sc["cloud"], gpu)
    rays, w = _t(sc["rays"], gpu), _t(r["weights"], gpu)
    V, H, W, P = rays.shape[0], sc["H"], sc["W"], x.shape[0]
    sizes = {"xyz": 3 * P, "density": P, "scaling": 3 * P, "rotation": 4 * P}
    stream = torch.cuda.current_stream(gpu).cuda_stream

    def call(V=V, H=H, P=P, rays=rays, means=x):
        buf = {k: _guarded(n, gpu) for k, n in sizes.items()}
        rc = L.r2_project_gaussians_fisher(V, H, W, None if rays is None else rays.data_ptr(), 1, P,
                                           None if means is None else means.data_ptr(), d.data_ptr(), s.data_ptr(), float(sc["mod"]),
                                           q.data_ptr(), w.data_ptr(), buf["xyz"][1].data_ptr(), buf["density"][1].data_ptr(),
                                           buf["scaling"][1].data_ptr(), buf["rotation"][1].data_ptr(), stream)
        torch.cuda.synchronize(gpu)
        return rc, buf

    rc, buf = call()
    assert rc == 0 and all(_intact(buf[k][0], n) for k, n in sizes.items())
    F = _fisher(sc, gpu, r["weights"])
    for k in R.GROUPS:
        assert torch.equal(buf[k][1].reshape(getattr(F, k).shape), getattr(F, k)), k
    for kw in (dict(V=0), dict(H=0), dict(P=-1), dict(rays=None), dict(means=None), dict(H=1 << 30)):
        rc, buf = call(**kw)
        assert rc == _lib.R2_ERR_INVALID and "r2_project_gaussians_fisher" in L.r2_last_error().decode(), kw
        assert all((buf[k][0] == SENTINEL).all() for k in sizes), kw
    rc, buf = call(P=0)
    assert rc == 0 and all((buf[k][0] == SENTINEL).all() for k in sizes)


def test_c_abi_of_the_variance_entries(gpu):
    """Guard words around both outputs; invalid arguments return R2_ERR_INVALID and write nothing; N = 0 returns 0 and touches
    nothing; P = 0 writes zeros."""
    from r2_gaussian_amd import _lib
    L = _lib.lib()
    stream = torch.cuda.current_stream(gpu).cuda_stream
    f = R.field_reference("tail_257")
    sc = f["scene"]
    x, d, s, q = _cloud(sc["cloud"], gpu)
    v = _var(f["var"], gpu)
    pts = _t(sc["points"].reshape(-1, 3), gpu)
    N, P = pts.shape[0], x.shape[0]
    n_points = N

    def query(N=N, P=P, pts=pts, vx=v[0]):
        whole, out = _guarded(n_points, gpu)
        rc = L.r2_query_gaussians_variance(N, None if pts is None else pts.data_ptr(), P, x.data_ptr(), d.data_ptr(), s.data_ptr(),
                                           float(sc["mod"]), q.data_ptr(), None if vx is None else vx.data_ptr(), v[1].data_ptr(),
                                           v[2].data_ptr(), v[3].data_ptr(), out.data_ptr(), stream)
        torch.cuda.synchronize(gpu)
        return rc, whole, out

    rc, whole, out = query()
    assert rc == 0 and _intact(whole, N) and torch.equal(out, _fvar(sc, f["var"], gpu))
    for kw in (dict(N=-1), dict(P=-1), dict(pts=None), dict(vx=None)):
        rc, whole, out = query(**kw)
        assert rc == _lib.R2_ERR_INVALID and "r2_query_gaussians_variance" in L.r2_last_error().decode(), kw
        assert (whole == SENTINEL).all(), kw
    rc, whole, out = query(N=0)
    assert rc == 0 and (whole == SENTINEL).all()
    rc, whole, out = query(P=0)
    assert rc == 0 and _intact(whole, N) and (out == 0).all()

    r = R.projector_reference("cone_p300_small")
    sc = r["scene"]
    x, d, s, q = _cloud(sc["cloud"], gpu)
    v = _var(r["var"], gpu)
    rays = _t(sc["rays"], gpu)
    V, H, W, P = rays.shape[0], sc["H"], sc["W"], x.shape[0]
    n_pixels = V * H * W

    def project(V=V, W=W, P=P, rays=rays, vq=v[3]):
        whole, out = _guarded(n_pixels, gpu)
        rc = L.r2_project_gaussians_variance(V, H, W, None if rays is None else rays.data_ptr(), 1, P, x.data_ptr(), d.data_ptr(),
                                             s.data_ptr(), float(sc["mod"]), q.data_ptr(), v[0].data_ptr(), v[1].data_ptr(),
                                             v[2].data_ptr(), None if vq is None else vq.data_ptr(), out.data_ptr(), stream)
        torch.cuda.synchronize(gpu)
        return rc, whole, out

    rc, whole, out = project()
    assert rc == 0 and _intact(whole, V * H * W) and torch.equal(out.reshape(V, H, W), _pvar(sc, r["var"], gpu))
    for kw in (dict(V=0), dict(W=0), dict(P=-1), dict(rays=None), dict(vq=None), dict(V=65536)):
        rc, whole, out = project(**kw)
        assert rc == _lib.R2_ERR_INVALID and "r2_project_gaussians_variance" in L.r2_last_error().decode(), kw
        assert (whole == SENTINEL).all(), kw
    rc, whole, out = project(P=0)
    assert rc == 0 and _intact(whole, V * H * W) and (out == 0).all()


# ------------------------------------------------------------------------------------------------------ the public layer
def test_end_to_end_next_best_view(gpu):
    """cone_p7: the Fisher diagonal of the three training views -> Laplace variances under a prior precision of 1e-3 -> the
    field variance on a plane and the information of four candidate views.  Everything finite and >= 0, and the candidate that
    is a training view scores lower than that view rotated by 90 degrees (in the float64 restatement by 15 %; the CPU test
    holds at least 10 %)."""
    from r2_gaussian_amd.field import plane_points
    from r2_gaussian_amd.uncertainty import (CloudTuple, field_variance, fisher_diagonal, parameter_variance, projection_variance,
                                             view_information)
    E = R.END_TO_END
    sc = R.proj_scene(E["scene"])
    cloud = _cloud(sc["cloud"], gpu)
    F = fisher_diagonal(sc["views"], *cloud)
    var = parameter_variance(F, E["prior"])
    assert isinstance(F, CloudTuple) and isinstance(var, CloudTuple)
    assert all(torch.isfinite(v).all() and (v > 0).all() for v in var)
    fv = field_variance(plane_points(device=gpu, **RF.PLANE), *cloud, var)
    assert fv.shape == (RF.PLANE["H"], RF.PLANE["W"]) and torch.isfinite(fv).all() and (fv >= 0).all() and (fv > 0).any()
    pv = projection_variance(sc["views"], *cloud, var)
    assert torch.isfinite(pv).all() and (pv >= 0).all() and (pv > 0).any()
    cand = R.candidate_views()
    score = view_information(cand, *cloud, var)
    want = R.information64()
    print("view information: kernels %s, float64 %s" % (score.cpu().numpy(), want))
    assert score.shape == (4,) and score.dtype == torch.float64 and torch.isfinite(score).all() and (score >= 0).all()
    assert score[E["seen"]] < score[E["unseen"]]


def test_argument_errors(gpu):
    from r2_gaussian_amd.uncertainty import field_variance, fisher_diagonal, fisher_diagonal_rays, projection_variance
    r = R.projector_reference("cone_p7")
    sc = r["scene"]
    x, d, s, q = _cloud(sc["cloud"], gpu)
    var = _var(r["var"], gpu)
    v = sc["views"]
    with pytest.raises(ValueError):
        fisher_diagonal(v, x.cpu(), d, s, q)
    with pytest.raises(ValueError):
        fisher_diagonal(v, x, d, s[:5], q)
    with pytest.raises(ValueError):
        fisher_diagonal([], x, d, s, q)
    with pytest.raises(ValueError):
        fisher_diagonal(v, x, d, s, q, weights=torch.ones((3, 17, 22), device=gpu))
    with pytest.raises(ValueError):
        fisher_diagonal_rays(np.zeros((2, 11), np.float32), True, 8, 8, x, d, s, q)
    with pytest.raises(ValueError):
        projection_variance(v, x, d, s, q, var[:3])
    with pytest.raises(ValueError):
        projection_variance(v, x, d, s, q, (var[0], var[1], var[2], var[3][:, :3]))
    pts = torch.zeros((5, 3), device=gpu)
    with pytest.raises(ValueError):
        field_variance(pts[:, :2], x, d, s, q, var)
    with pytest.raises(ValueError):
        field_variance(pts, x, d, s, q, tuple(a.cpu() for a in var))
    assert field_variance(pts[:0], x, d, s, q, var).shape == (0,)
    assert not fisher_diagonal(v, x.requires_grad_(True), d, s, q).xyz.requires_grad


def test_train_save_uncertainty(gpu, tmp_path):
    """``--save_uncertainty`` on the 32^3 blob of the trainer tests, ten iterations: fisher.npz and vol_std.npy appear in the last
    point_cloud directory with the right shapes, finite and >= 0."""
    from r2_gaussian_amd import datagen as D
    from r2_gaussian_amd import scene as S
    from r2_gaussian_amd import train as TR
    n = 32
    ax = -1 + (np.arange(n) + 0.5) * 2.0 / n
    X, Y, Z = np.meshgrid(ax, ax, ax, indexing="ij")
    vol = (0.6 * np.exp(-((X - 0.1) ** 2 + (Y + 0.2) ** 2 + Z ** 2) / (2 * 0.3 ** 2))).astype(np.float32)
    cfg = dict(S.CONE_BEAM, nVoxel=[n, n, n], nDetector=[32, 32], noise=False, totalAngle=360.0, startAngle=0.0)
    case = D.generate(vol, cfg, str(tmp_path / "data"), "blob", n_train=6, n_test=3, seed=0)
    out = TR.main(["-s", case, "-m", str(tmp_path / "model"), "--iterations", "10", "--test_iterations", "10", "--quiet",
                   "--save_uncertainty", "1e-3"])
    pc = tmp_path / "model" / "point_cloud" / "iteration_10"
    assert sorted(os.listdir(pc)) == sorted(["point_cloud.pickle", "vol_gt.npy", "vol_pred.npy", "fisher.npz", "vol_std.npy"])
    F = np.load(pc / "fisher.npz")
    P = out["P"]
    assert sorted(F.files) == sorted(R.GROUPS)
    for k, cols in zip(R.GROUPS, (3, 1, 3, 4)):
        assert F[k].shape == (P, cols) and F[k].dtype == np.float32 and np.isfinite(F[k]).all() and (F[k] >= 0).all()
    assert (F["density"] > 0).any()
    std = np.load(pc / "vol_std.npy")
    assert std.shape == (n, n, n) and std.dtype == np.float32 and np.isfinite(std).all() and (std >= 0).all() and (std > 0).any()
