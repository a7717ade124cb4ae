"""GPU: the Jacobian products of the exact projector (r2_project_gaussians_jvp, r2_project_gaussians_ray_jacobian;
csrc/gaussian_tangent.hip) against the float64 restatement of their contract (tests/gaussian_tangent_ref.py), and the two
Gauss-Newton solvers on top of them against their host loops.

Tolerance of a pixel (and component): 4 x e32 x normaliser + tail + the float32 underflow floor of gaussian_project_ref.
e32 is the measured error of the float32 restatement for that scene and quantity (tests/golden/gaussian_tangent/e32.json; the
CPU test holds every 4 x e32 below 1), the normaliser the float64 sum over the pixel's pairs of the addends' magnitudes, and
the factor 4 covers the device's expf / sqrt against numpy's.  tail is the float64 sum of the magnitudes of the pairs with
q > 32, which the contract lets the kernels sum or skip: these sums are signed, so there is no monotone bracket.  No pixel
or component is excluded.
"""
import numpy as np
import pytest
import torch

from tests import gaussian_project_rays_ref as RR
from tests import gaussian_project_ref as RP
from tests import gaussian_tangent_ref as R

pytestmark = pytest.mark.gpu

E32 = R.load_e32()
GUARD = 16          # guard words on either side of every buffer the C ABI writes
SENTINEL = -7.25


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _cloud(cloud, dev):
    return [_t(a, dev) for a in cloud]


def _tan(tan, dev):
    return tuple(_t(tan[k], dev) for k in R.GROUPS)


def _jvp(sc, tan, dev, rays=None, cloud=None, ray_tangent=None):
    from r2_gaussian_amd.gaussian_projector import project_gaussians_rays_jvp
    return project_gaussians_rays_jvp(_t(sc["rays"] if rays is None else rays, dev), sc["cone"], sc["H"], sc["W"],
                                      *_cloud(sc["cloud"] if cloud is None else cloud, dev),
                                      tangents=None if tan is None else _tan(tan, dev), ray_tangent=ray_tangent,
                                      scale_modifier=sc["mod"])


def _jac(sc, dev, rays=None, cloud=None):
    from r2_gaussian_amd.geometry import ray_jacobian
    return ray_jacobian(_t(sc["rays"] if rays is None else rays, dev), sc["cone"], sc["H"], sc["W"],
                        *_cloud(sc["cloud"] if cloud is None else cloud, dev), scale_modifier=sc["mod"])


def _project(sc, dev):
    from r2_gaussian_amd.gaussian_projector import project_gaussians_rays
    return project_gaussians_rays(_t(sc["rays"], dev), sc["cone"], sc["H"], sc["W"], *_cloud(sc["cloud"], dev), scale_modifier=sc["mod"])


# ------------------------------------------------------------------------------------------------------ against float64
@pytest.mark.parametrize("name", R.SCENES)
def test_jvp_vs_float64(gpu, name):
    """Entry 1 on every scene of gaussian_fisher_ref.PROJ_SCENES (detectors that are no multiple of the tile, 300 Gaussians on
    one tile, a Gaussian covering the detector, off it, behind and containing the source, raw quaternion norms, scale_modifier
    0.5, sigma 0.01 from six units away, P = 1), pixel by pixel."""
    r = R.reference(name)
    sc = r["scene"]
    out = _jvp(sc, r["tan"], gpu)
    assert out.shape == (sc["rays"].shape[0], sc["H"], sc["W"]) and out.dtype == torch.float32 and not out.requires_grad
    R.check(out.cpu().numpy(), r["jvp"], E32["jvp"][name], name + " jvp")


@pytest.mark.parametrize("name", R.SCENES)
def test_ray_jacobian_vs_float64(gpu, name):
    """Entry 2 on the same scenes, all six planes of every pixel."""
    r = R.reference(name)
    sc = r["scene"]
    out = _jac(sc, gpu)
    assert out.shape == (sc["rays"].shape[0], 6, sc["H"], sc["W"]) and out.dtype == torch.float32
    R.check(out.cpu().numpy(), r["jac"], E32["ray_jacobian"][name], name + " ray jacobian")


# ------------------------------------------------------------------------------------------------------ identities to rounding
@pytest.mark.parametrize("name", R.IDENTITY_SCENES)
def test_adjoint_identity(gpu, name):
    """<G, J t> = <J^T G, t> with r2_project_gaussians_backward's J^T G: the same pairs added in two orders by two kernels, both
    inner products accumulated in float64 on the host.  Tolerance: the sum of both sides' 4 x e32 x normalisers -- for the
    left side sum_pixels |G| N_pixel with the JVP's e32, for the right side sum_it |t| gabs_it with the backward's e32 of the
    group (tests/golden/gaussian_project/e32.json).  No tail: both kernels take the forward's pairs."""
    r = R.reference(name)
    sc = r["scene"]
    G = sc["G"].astype(np.float64)
    left = float((G * _jvp(sc, r["tan"], gpu).cpu().numpy().astype(np.float64)).sum())
    leaves = [t.requires_grad_(True) for t in _cloud(sc["cloud"], gpu)]
    from r2_gaussian_amd.gaussian_projector import project_gaussians_rays
    img = project_gaussians_rays(_t(sc["rays"], gpu), sc["cone"], sc["H"], sc["W"], *leaves, scale_modifier=sc["mod"])
    grads = torch.autograd.grad(img, leaves, _t(sc["G"], gpu))
    right = sum(float((g.cpu().numpy().astype(np.float64).reshape(r["tan"][k].shape) * r["tan"][k].astype(np.float64)).sum())
                for g, k in zip(grads, R.GROUPS))
    ref = RP.reference(name)["hi"]
    e_bwd = RP.load_e32()[name]
    tol = 4.0 * E32["jvp"][name] * float((np.abs(G) * r["jvp"]["N"]).sum())
    tol += sum(4.0 * e_bwd[k] * float((np.abs(r["tan"][k].astype(np.float64)) * ref["gabs"][k].reshape(r["tan"][k].shape)).sum())
               for k in R.GROUPS)
    want = float((G * r["jvp"]["out"]).sum())
    print("%s adjoint: <G, J t> %.9e, <J^T G, t> %.9e, difference %.3e, tolerance %.3e, float64 %.9e" % (name, left, right, abs(left - right), tol, want))
    assert abs(left) > 0 and abs(left - right) <= tol


@pytest.mark.parametrize("name", ["cone_p7", "parallel_p300", "cone_wide"])
def test_ray_jacobian_contracted_with_G_is_the_rays_backward(gpu, name):
    """The six planes contracted with G by pixel_ray_grad's rule and added over the pixels in float64 on the host reproduce
    r2_project_gaussians_rays_backward within both tolerances: 4 x e32 of the Jacobian x its normalisers chained the same way,
    and 4 x e32 of the ray gradient x its sum of |contributions| (gaussian_project_rays_ref).  No tail: both kernels take the
    forward's pairs."""
    from r2_gaussian_amd.gaussian_projector import project_gaussians_rays
    r = R.reference(name)
    sc = r["scene"]
    got = R.contract_with_pixel_gradient(_jac(sc, gpu).cpu().numpy(), sc["G"], sc["cone"])
    rays = _t(sc["rays"], gpu).requires_grad_(True)
    img = project_gaussians_rays(rays, sc["cone"], sc["H"], sc["W"], *_cloud(sc["cloud"], gpu), scale_modifier=sc["mod"])
    want = torch.autograd.grad(img, rays, _t(sc["G"], gpu))[0].cpu().numpy().astype(np.float64)
    absG = np.abs(sc["G"]).astype(np.float64)
    # |.| of pixel_ray_grad's rule, written as the parallel rule (planes 0..2 -> the pixel point, planes 3..5 -> a): in cone
    # beam the pixel point receives gd and the source a receives gs - gd, whose bound is the sum of both
    both = lambda A: np.concatenate([A[:, 3:6], A[:, 0:3] + A[:, 3:6]], 1) if sc["cone"] else A
    chain = lambda A: R.contract_with_pixel_gradient(both(A), absG, False)
    tol = 4.0 * E32["ray_jacobian"][name] * chain(r["jac"]["N"])
    tol = tol + 4.0 * RR.load_e32()[name] * RR.reference(name)["hi"]["gabs"] + R.FLOOR
    err = np.abs(got - want)
    print("%s: worst |contracted jacobian - rays backward| in units of the tolerance %.3f" % (name, (err / tol).max()))
    assert np.abs(want).max() > 0 and (err <= tol).all()


@pytest.mark.parametrize("name", ["cone_p7", "parallel_p300", "cone_stack300", "cone_mod"])
def test_a_density_tangent_gives_the_forward_image(gpu, name):
    """The image is linear in the densities: the tangent (0, density, 0, 0) gives the image itself, within the JVP's
    tolerance for that tangent (its normaliser is the sum of |terms|, gaussian_project_ref's `abs`) plus the forward's own
    4 x e32 x sum |terms|.  No tail: both kernels take the same pairs."""
    sc = RP.reference(name)["scene"]
    ref = RP.reference(name)
    tan = {"xyz": np.zeros_like(sc["cloud"][0]), "density": sc["cloud"][1].copy(), "scaling": np.zeros_like(sc["cloud"][2]),
           "rotation": np.zeros_like(sc["cloud"][3])}
    got, img = _jvp(sc, tan, gpu).cpu().numpy().astype(np.float64), _project(sc, gpu).cpu().numpy().astype(np.float64)
    tol = 4.0 * (E32["jvp"][name] + RP.load_e32()[name]["image"]) * ref["hi"]["abs"] + R.FLOOR
    print("%s: worst |jvp(density) - image| in units of the tolerance %.3f" % (name, (np.abs(got - img) / tol).max()))
    assert img.max() > 0 and (np.abs(got - img) <= tol).all()


# ------------------------------------------------------------------------------------------------------ bit identities
def test_calls_are_reproducible(gpu):
    r = R.reference("cone_p300")
    sc = r["scene"]
    assert torch.equal(_jvp(sc, r["tan"], gpu), _jvp(sc, r["tan"], gpu))
    assert torch.equal(_jac(sc, gpu), _jac(sc, gpu))


def test_doubling_the_tangent_doubles_the_output_exactly(gpu):
    r = R.reference("cone_p300")
    sc = r["scene"]
    one = _jvp(sc, r["tan"], gpu)
    assert (one != 0).any() and torch.equal(_jvp(sc, {k: 2.0 * v for k, v in r["tan"].items()}, gpu), 2.0 * one)


def test_a_zero_tangent_gives_exact_zeros(gpu):
    r = R.reference("cone_p7")
    sc = r["scene"]
    out = _jvp(sc, {k: np.zeros_like(v) for k, v in r["tan"].items()}, gpu)
    assert (out == 0).all() and not torch.signbit(out).any()


@pytest.mark.parametrize("name", ["cone_offdet", "parallel_offdet", "cone_behind"])
def test_the_tangent_of_an_unstaged_gaussian_is_never_read(gpu, name):
    """A NaN tangent on the Gaussian that projects off the detector, or lies behind the cone source, leaves the image finite
    and bit-identical; and the ray Jacobian is bit-identical to the one without that Gaussian."""
    r = R.reference(name)
    sc = r["scene"]
    assert sc["zero"]
    tan = {k: v.copy() for k, v in r["tan"].items()}
    for v in tan.values():
        v[sc["zero"]] = np.nan
    out = _jvp(sc, tan, gpu)
    assert torch.isfinite(out).all() and torch.equal(out, _jvp(sc, r["tan"], gpu)) and (out != 0).any()
    keep = [i for i in range(sc["cloud"][0].shape[0]) if i not in sc["zero"]]
    assert torch.equal(_jac(sc, gpu), _jac(sc, gpu, cloud=tuple(a[keep] for a in sc["cloud"])))


def test_an_appended_view_changes_no_bit_of_the_earlier_views(gpu):
    r = R.reference("cone_p7")
    sc = r["scene"]
    from tests import gaussian_fisher_ref as RFI
    from r2_gaussian_amd import projector
    extra = projector.ray_params(RFI.candidate_views("cone_p7", (1.2,)), (1.0, 1.0, 1.0), (0.0, 0.0, 0.0), (1, 1, 1))
    more = np.concatenate([sc["rays"], extra], 0)
    V = sc["rays"].shape[0]
    assert torch.equal(_jvp(sc, r["tan"], gpu, rays=more)[:V], _jvp(sc, r["tan"], gpu))
    assert torch.equal(_jac(sc, gpu, rays=more)[:V], _jac(sc, gpu))


def test_both_tangents_give_the_sum_of_the_parts(gpu):
    """project_gaussians_rays_jvp with a cloud tangent and a ray tangent = the float32 sum of the two calls, bit for bit; and
    the ray part is the float64 contraction of the restatement within the Jacobian's tolerance chained through |ds|, |dd|."""
    r = R.reference("cone_p7")
    sc = r["scene"]
    rt = (0.01 * np.random.RandomState(9).randn(*sc["rays"].shape)).astype(np.float32)
    a, b = _jvp(sc, r["tan"], gpu), _jvp(sc, None, gpu, ray_tangent=_t(rt, gpu))
    assert b.dtype == torch.float32 and (b != 0).any()
    assert torch.equal(_jvp(sc, r["tan"], gpu, ray_tangent=rt), a + b)
    want = R.contract_jacobian(r["jac"]["out"], rt, sc["cone"])
    art = np.abs(rt).astype(np.float64)
    # cone: Js . ta + Jd . (tP - ta) is bounded by Nd |tP| + (Ns + Nd) |ta|, which is the parallel rule on [Nd, Ns + Nd]
    bound = lambda A: R.contract_jacobian(np.concatenate([A[:, 3:6], A[:, 0:3] + A[:, 3:6]], 1), art, False)
    tol = 4.0 * E32["ray_jacobian"]["cone_p7"] * bound(r["jac"]["N"]) + bound(r["jac"]["tail"]) + 2.0 ** -22 * np.abs(want) + R.FLOOR
    assert (np.abs(b.cpu().numpy().astype(np.float64) - want) <= tol).all()


# ------------------------------------------------------------------------------------------------------ the solvers
def test_geometry_lm_follows_the_host_loop(gpu):
    """refine_geometry_lm on cone_p7's geometry, the projections measured with the detector shifted by 1.5 pixels, 3 iterations
    from offDetector = 0.  The reference module runs the same loop on the host in float64 and in float32
    (tests/golden/gaussian_tangent/refine_lm.json; the CPU tests re-measure it and check that the float64 loop ends below
    the Adam loop's error after 60 steps).  The GPU's final offDetector must lie within 4 x max |float32 loop - float64 loop| of
    the float64 loop's, in the maximum norm over the two parameters."""
    from r2_gaussian_amd.geometry import refine_geometry_lm
    gold = R.load_refine_lm()
    st = RR.refine_setup()
    projs = torch.from_numpy(st["projs"]).to(gpu)
    start = {"offDetector": torch.zeros(2, dtype=torch.float64, device=gpu)}
    got, hist = refine_geometry_lm(projs, _cloud(st["cloud"], gpu), RR.refine_rays_fn(st, gpu), start, gold["iters"], gold["damping"])
    assert (start["offDetector"] == 0).all() and hist.shape == (gold["iters"],) and hist.is_cuda
    p = got["offDetector"].cpu().numpy()
    dist, tol = float(np.abs(p - np.asarray(gold["final64"])).max()), 4.0 * gold["f32_minus_f64"]
    print("geometry LM: offDetector %s, float64 loop %s, distance %.3e, tolerance %.3e; loss %s (float64 loop %s)"
          % (p, gold["final64"], dist, tol, hist.cpu().numpy(), gold["loss64"]))
    assert dist <= tol


def test_refine_cloud_follows_the_host_loop(gpu):
    """refine_cloud on cone_p7 perturbed by 0.03 randn (gaussian_tangent_ref.gauss_newton_setup), 3 LM steps with the recorded
    cg_iters: the final loss lies within 4 x |float32 loop - float64 loop| of the float64 loop's
    (tests/golden/gaussian_tangent/gauss_newton.json) and below a tenth of the initial loss."""
    from r2_gaussian_amd.gauss_newton import refine_cloud
    from r2_gaussian_amd.gaussian_projector import project_gaussians_rays
    gold = R.load_gauss_newton()
    st = R.gauss_newton_setup()
    projs, rays = _t(st["projs"], gpu), _t(st["rays"], gpu)
    cloud, hist = refine_cloud(rays, projs, _cloud(st["start"], gpu), gold["steps"], gold["cg_iters"], gold["damping"], cone=True,
                               max_log_step=gold["max_log_step"])
    assert hist.shape == (gold["steps"],) and hist.is_cuda and all(c.dtype == torch.float32 for c in cloud)
    res = (project_gaussians_rays(rays, True, st["H"], st["W"], *cloud) - projs).to(torch.float64)
    final, first = float((res * res).mean()), float(hist[0])
    dist, tol = abs(final - gold["loss64"][-1]), 4.0 * gold["f32_minus_f64"]
    print("cloud LM: loss %s -> %.9e, float64 loop %s, distance %.3e, tolerance %.3e" % (hist.cpu().numpy(), final, gold["loss64"], dist, tol))
    assert final < 0.1 * first
    assert (cloud[1] > 0).all() and (cloud[2] > 0).all()
    assert dist <= tol


def test_normal_matvec_is_jvp_then_backward(gpu):
    """normal_matvec = J^T (w * J t) + damping F t, assembled from the public pieces, bit for bit."""
    from r2_gaussian_amd.gauss_newton import normal_matvec
    from r2_gaussian_amd.gaussian_projector import project_gaussians_rays
    from r2_gaussian_amd.uncertainty import fisher_diagonal_rays
    from tests import gaussian_fisher_ref as RFI
    r = R.reference("cone_p7")
    sc = r["scene"]
    rays, cloud, tan = _t(sc["rays"], gpu), _cloud(sc["cloud"], gpu), _tan(r["tan"], gpu)
    w = _t(RFI.scene_weights(sc["rays"].shape[0], sc["H"], sc["W"]), gpu)
    out = normal_matvec(rays, sc["cone"], sc["H"], sc["W"], cloud, tan, weights=w, damping=0.5)
    jt = _jvp(sc, r["tan"], gpu)
    leaves = [t.clone().requires_grad_(True) for t in cloud]
    grads = torch.autograd.grad(project_gaussians_rays(rays, sc["cone"], sc["H"], sc["W"], *leaves), leaves, jt * w)
    F = fisher_diagonal_rays(rays, sc["cone"], sc["H"], sc["W"], *cloud, weights=w)
    for o, g, f, t in zip(out, grads, F, tan):
        assert torch.equal(o, g.reshape(o.shape) + 0.5 * f.reshape(o.shape) * t.reshape(o.shape))
    assert all((o != 0).any() for o in out)


# ------------------------------------------------------------------------------------------------------ the C ABI itself
def _guarded(n, dev):
    whole = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.float32, device=dev)
    return whole, whole[GUARD:GUARD + n]


def _intact(whole, n):
    return bool((whole[:GUARD] == SENTINEL).all()) and bool((whole[GUARD + n:] == SENTINEL).all())


def test_c_abi_of_both_entries(gpu):
    """Through ctypes: guard words around both outputs survive and the public layer returns the C entries' bits; invalid
    arguments return R2_ERR_INVALID, name the entry and write nothing; P = 0 writes zeros."""
    from r2_gaussian_amd import _lib
    L = _lib.lib()
    stream = torch.cuda.current_stream(gpu).cuda_stream
    r = R.reference("cone_p300_small")
    sc = r["scene"]
    x, d, s, q = _cloud(sc["cloud"], gpu)
    t = _tan(r["tan"], gpu)
    rays = _t(sc["rays"], gpu)
    V, H, W, P = rays.shape[0], sc["H"], sc["W"], x.shape[0]

    def jvp(V=V, W=W, P=P, rays=rays, tq=t[3], means=x):
        whole, out = _guarded(V * H * W if 0 < V < 100 and W > 0 else 1, gpu)
        rc = L.r2_project_gaussians_jvp(V, H, W, None if rays is None else rays.data_ptr(), 1, P,
                                        None if means is None else means.data_ptr(), d.data_ptr(), s.data_ptr(), float(sc["mod"]),
                                        q.data_ptr(), t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(),
                                        None if tq is None else tq.data_ptr(), out.data_ptr(), stream)
        torch.cuda.synchronize(gpu)
        return rc, whole, out

    rc, whole, out = jvp()
    assert rc == 0 and _intact(whole, V * H * W) and torch.equal(out.reshape(V, H, W), _jvp(sc, r["tan"], gpu))
    for kw in (dict(V=0), dict(W=0), dict(P=-1), dict(rays=None), dict(tq=None), dict(means=None), dict(V=65536)):
        rc, whole, out = jvp(**kw)
        assert rc == _lib.R2_ERR_INVALID and "r2_project_gaussians_jvp" in L.r2_last_error().decode(), kw
        assert (whole == SENTINEL).all(), kw
    rc, whole, out = jvp(P=0)
    assert rc == 0 and _intact(whole, V * H * W) and (out == 0).all()

    def jac(V=V, W=W, P=P, rays=rays, means=x, null_out=False):
        whole, out = _guarded(V * 6 * H * W if 0 < V < 100 and W > 0 else 1, gpu)
        rc = L.r2_project_gaussians_ray_jacobian(V, H, W, None if rays is None else rays.data_ptr(), 1, P,
                                                 None if means is None else means.data_ptr(), d.data_ptr(), s.data_ptr(),
                                                 float(sc["mod"]), q.data_ptr(), None if null_out else out.data_ptr(), stream)
        torch.cuda.synchronize(gpu)
        return rc, whole, out

    rc, whole, out = jac()
    assert rc == 0 and _intact(whole, V * 6 * H * W) and torch.equal(out.reshape(V, 6, H, W), _jac(sc, gpu))
    for kw in (dict(V=0), dict(W=0), dict(P=-1), dict(rays=None), dict(means=None), dict(null_out=True), dict(V=65536)):
        rc, whole, out = jac(**kw)
        assert rc == _lib.R2_ERR_INVALID and "r2_project_gaussians_ray_jacobian" in L.r2_last_error().decode(), kw
        assert (whole == SENTINEL).all(), kw
    rc, whole, out = jac(P=0)
    assert rc == 0 and _intact(whole, V * 6 * H * W) and (out == 0).all()


def test_argument_errors(gpu):
    from r2_gaussian_amd.gauss_newton import gauss_newton_step, normal_matvec, refine_cloud
    from r2_gaussian_amd.gaussian_projector import project_gaussians_jvp, project_gaussians_rays_jvp
    from r2_gaussian_amd.geometry import ray_jacobian, refine_geometry_lm
    r = R.reference("cone_p7")
    sc = r["scene"]
    x, d, s, q = _cloud(sc["cloud"], gpu)
    tan = _tan(r["tan"], gpu)
    v, rays = sc["views"], _t(sc["rays"], gpu)
    H, W = sc["H"], sc["W"]
    with pytest.raises(ValueError):
        project_gaussians_jvp(v, x, d, s, q)                                   # neither tangent
    with pytest.raises(ValueError):
        project_gaussians_jvp(v, x, d, s, q, tangents=tan[:3])
    with pytest.raises(ValueError):
        project_gaussians_jvp(v, x, d, s, q, tangents=(tan[0], tan[1], tan[2], tan[3][:, :3]))
    with pytest.raises(ValueError):
        project_gaussians_jvp(v, x, d, s, q, tangents=tuple(a.cpu() for a in tan))
    with pytest.raises(ValueError):
        project_gaussians_jvp(v, x.cpu(), d, s, q, tangents=tan)
    with pytest.raises(ValueError):
        project_gaussians_jvp([], x, d, s, q, tangents=tan)
    with pytest.raises(ValueError):
        project_gaussians_rays_jvp(rays, True, H, W, x, d, s, q, ray_tangent=torch.zeros((2, 12)))
    with pytest.raises(ValueError):
        ray_jacobian(np.zeros((2, 11), np.float32), True, 8, 8, x, d, s, q)
    with pytest.raises(ValueError):
        ray_jacobian(rays, True, H, W, x, d, s[:5], q)
    with pytest.raises(ValueError):
        normal_matvec(rays, True, H, W, (x, d, s, q), tan, weights=torch.ones((3, 17, 22), device=gpu))
    projs = torch.zeros((3, H, W), device=gpu)
    with pytest.raises(ValueError):
        gauss_newton_step(rays, True, H, W, (x, d, s, q), projs[:2], 2, 1e-3)
    with pytest.raises(ValueError):
        gauss_newton_step(rays, True, H, W, (x, d, s, q), projs, 0, 1e-3)
    with pytest.raises(ValueError):
        gauss_newton_step(rays, True, H, W, (x, d, s, q), projs, 2, 1e-3, max_log_step=0.0)
    with pytest.raises(ValueError):
        refine_cloud(rays, projs.cpu(), (x, d, s, q), 1, 2)
    with pytest.raises(ValueError):
        refine_cloud(rays, projs[:2], (x, d, s, q), 1, 2)
    with pytest.raises(ValueError):
        refine_geometry_lm(projs.cpu(), (x, d, s, q), lambda p: rays, {"offDetector": torch.zeros(2, device=gpu)}, 1)
    with pytest.raises(ValueError):
        refine_geometry_lm(projs, (x, d, s, q), lambda p: rays, {}, 1)
    assert not project_gaussians_jvp(v, x.requires_grad_(True), d, s, q, tangents=tan).requires_grad
