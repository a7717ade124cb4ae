"""GPU: the exact Gaussian projector (r2_gaussian_amd.gaussian_projector; csrc/gaussian_project.hip and its backward) against
the float64 restatement of its contract (tests/gaussian_project_ref.py).

Tolerance: 4 x e32 x sum_g |term_g| per pixel (and 4 x e32_k x sum_pairs |contribution| per gradient component), e32 being
the measured error of the float32 restatement against float64 for that scene (tests/golden/gaussian_project/e32.json; the
factor 4 covers the device's expf / sqrt / division against numpy's and the different association of the sums), plus the
float32 underflow floor of the reference module.  Bracket: the contract lets a pair with q > 32 be summed or skipped, so the
kernel must lie between the float64 sum cut at q <= 32 and the float64 sum of every pair, each widened by the tolerance, at
every pixel and every gradient component; none is excluded.
"""
import numpy as np
import pytest
import torch

from tests import gaussian_project_ref as R

pytestmark = pytest.mark.gpu

E32 = R.load_e32()


def _leaves(cloud, dev, grad=False):
    return [torch.from_numpy(a).to(dev).requires_grad_(grad) for a in cloud]


def _project(sc, dev, grad=False, views=None):
    from r2_gaussian_amd.gaussian_projector import project_gaussians
    leaves = _leaves(sc["cloud"], dev, grad)
    img = project_gaussians(sc["views"] if views is None else views, *leaves, scale_modifier=sc["mod"])
    return img, leaves


def _bracket(got, a, b, tol, what):
    got = np.asarray(got, np.float64).reshape(a.shape)
    lo, hi = np.minimum(a, b) - tol, np.maximum(a, b) + tol
    bad = (got < lo) | (got > hi) | ~np.isfinite(got)
    worst = float(np.max(np.maximum(lo - got, got - hi) / np.maximum(tol, 1e-300)))
    print("%s: worst excess over the bracket in units of the tolerance %.3f (1 + this <= 1 passes)" % (what, worst))
    assert not bad.any(), "%s: %d of %d outside the bracket, worst excess %.3g tolerances" % (what, int(bad.sum()), bad.size, worst)


def _check_image(name, img):
    r = R.reference(name)
    tol = 4.0 * E32[name]["image"] * r["hi"]["abs"] + R.FLOOR
    _bracket(img.detach().cpu().numpy(), r["lo"]["img"], r["hi"]["img"], tol, name + " image")


def _check_grads(name, leaves):
    r = R.reference(name)
    for k, t in zip(R.GRADS, leaves):
        tol = 4.0 * E32[name][k] * r["hi"]["gabs"][k] + R.FLOOR
        _bracket(t.grad.cpu().numpy(), r["lo"]["grads"][k], r["hi"]["grads"][k], tol, name + " d" + k)


FORWARD = [b + "_" + k for b in ("cone", "parallel") for k in R.MAIN + R.EDGE + ("small_sigma",)] + ["cone_behind", "cone_contains"]


@pytest.mark.parametrize("name", FORWARD)
def test_forward_and_backward_vs_float64(gpu, name):
    """Image and all four gradients (autograd end to end: loss = sum(G * image), .backward(), grads on the leaves) inside
    the float64 bracket: P in {1, 7, 300}, detectors 8x8, 17x23, 70x50, V in {1, 3}, scales 0.01 .. 0.5 with a 50:1
    Gaussian, and the edge scenes (whole detector, off the detector, 300 on one tile, quaternion norms 2 / 0.5 / 1.3,
    scale_modifier 0.5, sigma 0.01 with the source six units away, behind the source, sphere around the source)."""
    sc = R.reference(name)["scene"]
    img, leaves = _project(sc, gpu, grad=True)
    assert img.shape == (len(sc["views"]), sc["H"], sc["W"]) and img.dtype == torch.float32
    _check_image(name, img)
    (img * torch.from_numpy(sc["G"]).to(gpu)).sum().backward()
    _check_grads(name, leaves)


@pytest.mark.parametrize("name", ["cone_offdet", "parallel_offdet", "cone_behind"])
def test_untouched_gaussians_contribute_exact_zeros(gpu, name):
    """A Gaussian that projects off the detector, or lies behind the cone source: the image is bit-identical to the one
    without it, and its gradients are exact zeros."""
    sc = R.reference(name)["scene"]
    img, leaves = _project(sc, gpu, grad=True)
    keep = [i for i in range(sc["cloud"][0].shape[0]) if i not in sc["zero"]]
    without = dict(sc, cloud=tuple(a[keep] for a in sc["cloud"]))
    img2, _ = _project(without, gpu)
    assert torch.equal(img.detach(), img2)
    (img * torch.from_numpy(sc["G"]).to(gpu)).sum().backward()
    for t in leaves:
        assert (t.grad[sc["zero"]] == 0).all() and torch.isfinite(t.grad).all()


def test_no_gaussians_writes_zeros(gpu):
    from r2_gaussian_amd.gaussian_projector import project_gaussians
    sc = R.scene("cone_p7")
    out = torch.full((3, 17, 23), 7.0, device=gpu)
    e = lambda c: torch.zeros((0, c), device=gpu)
    img = project_gaussians(sc["views"], e(3), e(1), e(3), e(4), out=out)
    assert img.data_ptr() == out.data_ptr() and (out == 0).all()


def test_degenerate_gaussians_write_zero(gpu):
    """A scale of 0, a negative scale and a NaN mean: those Gaussians contribute 0 and the rest of the image is untouched."""
    sc = R.scene("cone_p7")
    xyz, dens, scal, rot = (a.copy() for a in sc["cloud"])
    scal[1, 0], scal[2, 1], xyz[3, 2] = 0.0, -0.1, np.nan
    img, _ = _project(dict(sc, cloud=(xyz, dens, scal, rot)), gpu)
    keep = [0, 4, 5, 6]
    img2, _ = _project(dict(sc, cloud=tuple(a[keep] for a in sc["cloud"])), gpu)
    assert torch.isfinite(img).all() and torch.equal(img, img2)


@pytest.mark.parametrize("beam", ["cone", "parallel"])
def test_views_are_independent_and_calls_reproducible(gpu, beam):
    """Views [a, b, c] give bit-identical images to [b] alone; two forward calls and two backward calls give the same bits."""
    sc = R.scene(beam + "_p7")
    img, leaves = _project(sc, gpu, grad=True)
    one, _ = _project(sc, gpu, views=sc["views"][1:2])
    assert torch.equal(img[1].detach(), one[0])
    G = torch.from_numpy(sc["G"]).to(gpu)
    (img * G).sum().backward()
    img2, leaves2 = _project(sc, gpu, grad=True)
    assert torch.equal(img.detach(), img2.detach())
    (img2 * G).sum().backward()
    for a, b in zip(leaves, leaves2):
        assert torch.equal(a.grad, b.grad)


def test_caller_supplied_rays_match_the_views(gpu):
    from r2_gaussian_amd.gaussian_projector import project_gaussians_rays, world_ray_params
    sc = R.scene("cone_p7")
    img, _ = _project(sc, gpu)
    rays = world_ray_params(sc["views"])
    assert np.array_equal(rays, sc["rays"])
    img2 = project_gaussians_rays(rays, True, sc["H"], sc["W"], *_leaves(sc["cloud"], gpu))
    assert torch.equal(img, img2)


def _anchor_scene():
    """Eight well-separated small Gaussians, parallel beam along x on 64x64 (pixel pitch 1/32): two columns, four rows."""
    from r2_gaussian_amd import scene as S
    g = np.random.RandomState(3)
    xyz = np.array([[0.1 * g.randn(), y, z] for z in (-0.6, -0.2, 0.2, 0.6) for y in (-0.4, 0.4)], np.float32)
    sc = np.exp(np.log(0.03) + g.rand(8, 3) * np.log(2.0)).astype(np.float32)
    q = g.randn(8, 4)
    q = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)
    dens = (0.2 + 0.8 * g.rand(8, 1)).astype(np.float32)
    return S.make_view(0.0, (64, 64), S.PARALLEL_BEAM), (xyz, dens, sc, q)


def test_anchor_against_the_rasterizer_parallel(gpu):
    """Parallel beam, where splatting is exact up to its cut: every pair the rasterizer drops lies outside a square of
    half-side >= 3 sigma_max, so has q >= 9 and is below exp(-4.5) of that Gaussian's peak; hence
    |exact - raster| <= exp(-4.5) sum_g peak_g + tol at every pixel, and at the pixel nearest each Gaussian's centre the two
    agree within tol plus the other Gaussians' terms there.  tol = 4 e32 sum|term| with this scene's own measured e32."""
    from r2_gaussian_amd import GaussianRasterizationSettings, GaussianRasterizer
    from r2_gaussian_amd import projector
    from r2_gaussian_amd.gaussian_projector import project_gaussians
    v, cloud = _anchor_scene()
    leaves = _leaves(cloud, gpu)
    exact = project_gaussians([v], *leaves)[0].cpu().numpy().astype(np.float64)
    rs = GaussianRasterizationSettings(64, 64, v.tanfovx, v.tanfovy, 1.0, v.world_view_transform.to(gpu),
                                       v.full_proj_transform.to(gpu), v.camera_center.to(gpu), False, v.mode, False)
    raster, _ = GaussianRasterizer(rs)(leaves[0], torch.zeros_like(leaves[0]), leaves[1], scales=leaves[2], rotations=leaves[3])
    raster = raster.reshape(64, 64).cpu().numpy().astype(np.float64)
    rays = projector.ray_params([v], (1.0, 1.0, 1.0), (0.0, 0.0, 0.0), (1, 1, 1))
    r64 = R.project64(rays, False, 64, 64, *cloud)
    r32 = R.project32(rays, False, 64, 64, *cloud)
    e32 = R.error_against(r64, r32["img"])["image"]
    tol = 4.0 * e32 * r64["abs"][0] + R.FLOOR
    S, D = R.pixel_rays(rays, False, 64, 64, np.float64)
    s = [S[j][0].reshape(-1, 1) for j in range(3)]
    d = [D[j][0].reshape(-1, 1) for j in range(3)]
    o = R.contract(np, s, d, False, R._cols(cloud[0], np.float64), R._cols(cloud[1], np.float64)[0], R._cols(cloud[2], np.float64),
                   1.0, R._cols(cloud[3], np.float64))
    terms = o["term"]                                   # [pixels, 8]
    with np.errstate(all="ignore"):                     # (0 / 0 where exp(-q / 2) underflows)
        peaks = np.nanmax(terms / np.exp(-0.5 * o["q"]), 0)   # rho sqrt(2 pi / A) |d| per Gaussian
    diff = np.abs(exact - raster)
    print("anchor: max |exact - raster| %.3e, bound %.3e, image max %.3e" % (diff.max(), np.exp(-4.5) * peaks.sum(), exact.max()))
    assert (diff <= np.exp(-4.5) * peaks.sum() + tol).all()
    for g in range(8):
        pix = int(np.argmin(o["q"][:, g]))
        others = terms[pix].sum() - terms[pix, g]
        dd = diff.reshape(-1)[pix]
        print("anchor: Gaussian %d centre pixel %d: |exact - raster| %.3e, tol %.3e, others %.3e" % (g, pix, dd, tol.reshape(-1)[pix], others))
        assert dd <= tol.reshape(-1)[pix] + others


def test_consistent_with_the_volume_path(gpu):
    """Loose physical check: the Siddon projection of the voxelizer's query volume of a smooth cloud (scales >= 3 voxels on a
    48^3 grid, 32^2 detector, cone beam) against the exact projection of the same cloud.  The bound is not derived: the
    voxelizer samples the model at voxel centres and cuts it, Siddon integrates that piecewise-constant volume, and no
    closed bound for the two together is at hand.  The discrepancy measured for this scene with the CPU restatements of all
    three (the oracle's voxelizer, tests/siddon_ref.py in float64, tests/gaussian_project_ref.py in float64) is
    max |siddon - exact| = 1.46e-2 of the image maximum; this asserts 2 x that, 2.92e-2, of the
    kernels."""
    from r2_gaussian_amd import GaussianVoxelizationSettings, GaussianVoxelizer
    from r2_gaussian_amd import scene as S
    from r2_gaussian_amd.gaussian_projector import project_gaussians
    from r2_gaussian_amd.projector import project_views
    n = 48
    g = np.random.RandomState(9)
    xyz = ((g.rand(40, 3) * 2 - 1) * 0.35).astype(np.float32)
    sc = (3.0 * 2.0 / n * (1.0 + g.rand(40, 3))).astype(np.float32)   # 3 .. 6 voxels of 2 / 48
    q = g.randn(40, 4)
    q = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)
    dens = (0.1 + 0.4 * g.rand(40, 1)).astype(np.float32)
    leaves = _leaves((xyz, dens, sc, q), gpu)
    vs = GaussianVoxelizationSettings(1.0, n, n, n, 2.0, 2.0, 2.0, 0.0, 0.0, 0.0, False, False)
    vol, _ = GaussianVoxelizer(vs)(leaves[0], leaves[1], scales=leaves[2], rotations=leaves[3])
    views = [S.make_view(a, (32, 32)) for a in (0.4, 2.0)]
    sid = project_views(vol, views, (2.0, 2.0, 2.0), (0.0, 0.0, 0.0), projection_type="siddon")
    exact = project_gaussians(views, *leaves)
    rel = float((sid - exact).abs().max() / exact.max())
    print("volume path: max |siddon(query) - exact| / max(exact) = %.4e" % rel)
    assert rel <= 2.92e-2


def test_argument_errors(gpu):
    from r2_gaussian_amd import scene as S
    from r2_gaussian_amd.gaussian_projector import project_gaussians, project_gaussians_rays
    sc = R.scene("cone_p7")
    x, d, s, r = _leaves(sc["cloud"], gpu)
    v = sc["views"]
    with pytest.raises(ValueError):
        project_gaussians(v, x.cpu(), d, s, r)
    with pytest.raises(ValueError):
        project_gaussians(v, x, d, s[:5], r)
    with pytest.raises(ValueError):
        project_gaussians(v, x, d, s, r[:, :3])
    with pytest.raises(ValueError):
        project_gaussians(v, x, d[:3], s, r)
    with pytest.raises(ValueError):
        project_gaussians([v[0], S.make_view(0.1, (17, 23), S.PARALLEL_BEAM)], x, d, s, r)
    with pytest.raises(ValueError):
        project_gaussians([v[0], S.make_view(0.1, (16, 23))], x, d, s, r)
    with pytest.raises(ValueError):
        project_gaussians([], x, d, s, r)
    with pytest.raises(ValueError):
        project_gaussians(v, x, d, s, r, out=torch.empty((3, 17, 22), device=gpu))
    with pytest.raises(ValueError):
        project_gaussians_rays(np.zeros((2, 11), np.float32), True, 8, 8, x, d, s, r)
