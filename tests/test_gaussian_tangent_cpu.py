"""CPU: the restatement of the Jacobian-product entries (tests/gaussian_tangent_ref.py) against autograd's Jacobian and the
ray gradient's autograd, the measured float32 error the GPU tolerance is taken from, the header and the binding, and the two
host solver loops the GPU solvers are held against (tests/golden/gaussian_tangent/refine_lm.json, gauss_newton.json)."""
import os
import re

import numpy as np
import pytest
import torch

from tests import gaussian_project_rays_ref as RR
from tests import gaussian_project_ref as RP
from tests import gaussian_tangent_ref as R

ENTRIES = ("r2_project_gaussians_jvp", "r2_project_gaussians_ray_jacobian")


@pytest.mark.parametrize("name", ["cone_p1", "parallel_p1", "cone_p7"])
def test_jvp64_is_the_jacobian_applied_to_the_tangent(name):
    """The float64 restatement of r2_project_gaussians_jvp (every pair) = jacobian(torch_image) . t with the Jacobian from
    torch.autograd.functional.jacobian of gaussian_project_ref.torch_image, to 1e-10 of the pixel's normaliser."""
    r = R.reference(name)
    sc = r["scene"]
    f = lambda x, d, s, q: RP.torch_image(sc["rays"], sc["cone"], sc["H"], sc["W"], x, d, s, q, sc["mod"]).reshape(-1)
    leaves = tuple(torch.from_numpy(np.asarray(a, np.float64)) for a in sc["cloud"])
    J = torch.autograd.functional.jacobian(f, leaves)
    want = sum((j.reshape(j.shape[0], -1) @ torch.from_numpy(r["tan"][k].astype(np.float64)).reshape(-1)) for j, k in zip(J, R.GROUPS))
    want = want.numpy().reshape(r["jvp"]["out"].shape)
    assert np.abs(want).max() > 0
    assert (np.abs(r["jvp"]["out"] - want) <= 1e-10 * r["jvp"]["N"]).all()


@pytest.mark.parametrize("name", ["cone_p7", "parallel_p7", "cone_contains"])
def test_ray_jacobian64_contracted_with_G_is_the_ray_gradient(name):
    """The float64 ray Jacobian contracted with G by pixel_ray_grad's rule and added over the pixels equals
    gaussian_project_rays_ref.torch_ray_grad (autograd through the contract), to 1e-10 of the sum of |contributions|."""
    r = R.reference(name)
    sc = r["scene"]
    got = R.contract_with_pixel_gradient(r["jac"]["out"], sc["G"], sc["cone"])
    auto = RR.torch_ray_grad(sc["rays"], sc["cone"], sc["H"], sc["W"], *sc["cloud"], sc["mod"], sc["G"])
    gabs = RR.reference(name)["hi"]["gabs"]
    assert (gabs > 0).all() and (np.abs(got - auto) <= 1e-10 * gabs).all()


def test_contracting_with_a_ray_tangent_is_the_transpose_of_contracting_with_G():
    """<G, contract_jacobian(jac, t)> = <contract_with_pixel_gradient(jac, G), t>: the two chain rules the product and the
    tests use are each other's transposes, both beams."""
    for name in ("cone_p7", "parallel_p7"):
        r = R.reference(name)
        sc = r["scene"]
        t = np.random.RandomState(8).randn(*sc["rays"].shape)
        a = float((sc["G"].astype(np.float64) * R.contract_jacobian(r["jac"]["out"], t, sc["cone"])).sum())
        b = float((R.contract_with_pixel_gradient(r["jac"]["out"], sc["G"], sc["cone"]) * t).sum())
        assert abs(a) > 0 and abs(a - b) <= 1e-12 * (abs(a) + abs(b))


def test_stored_e32_matches_a_fresh_measurement():
    """tests/golden/gaussian_tangent/e32.json (python -m tests.gaussian_tangent_ref) within 10 % of a fresh measurement; every
    4 x e32 the tolerance uses stays below 1, so a kernel that is wrong by a factor cannot pass; and the two scenes whose ray
    Jacobian is normalised with the floor are exactly those whose plain 4 x e32 reaches 1."""
    stored, fresh = R.load_e32(), R.measure_e32()
    assert sorted(stored) == ["jvp", "ray_jacobian", "ray_jacobian_plain"]
    for q in stored:
        assert sorted(stored[q]) == sorted(R.SCENES)
        for n in R.SCENES:
            assert abs(stored[q][n] - fresh[q][n]) <= 0.1 * fresh[q][n], (q, n, stored[q][n], fresh[q][n])
    for n in R.SCENES:
        assert 4.0 * stored["jvp"][n] < 1.0 and 4.0 * stored["ray_jacobian"][n] < 1.0, n
        assert (4.0 * stored["ray_jacobian_plain"][n] >= 1.0) == (n in R.FLOORED_JAC), n


def test_header_declares_and_the_binding_binds_both_entries():
    from r2_gaussian_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "r2hip.h")) as f:
        header = f.read()
    assert "#define R2_ABI_VERSION 3" in header and _lib.R2_ABI_VERSION == 3   # the entries are additive
    for name in ENTRIES:
        assert re.search(r"R2_API int %s\(" % name, header), name
        assert name in _lib.exported_symbols()
    assert len(_lib._SIGNATURES["r2_project_gaussians_jvp"][1]) == 17
    assert len(_lib._SIGNATURES["r2_project_gaussians_ray_jacobian"][1]) == 13


def test_stored_geometry_lm_matches_a_fresh_run():
    """refine_lm.json: after LM_ITERS = 3 iterations the float64 loop's offset error lies below the Adam fixture's after its 60
    steps (tests/golden/gaussian_project_rays/refine.json: final_error64), the float32 and float64 loops take the same
    accept / reject sequence, the final parameters are reproduced, and the float32 loop's distance from the float64 one --
    the GPU test's tolerance is 4 x the stored one -- is reproduced within a factor 2."""
    stored, fresh = R.load_refine_lm(), R.measure_refine_lm()
    assert (stored["iters"], stored["damping"]) == (R.LM_ITERS, R.LM_DAMPING) == (3, 1e-3)
    assert stored["final_error64"] < RR.load_refine()["final_error64"]
    assert stored["accepts64"] == stored["accepts32"] == fresh["accepts64"] == fresh["accepts32"]
    assert np.allclose(stored["final64"], fresh["final64"], rtol=0, atol=1e-9)
    assert 0.5 * stored["f32_minus_f64"] <= fresh["f32_minus_f64"] <= 2.0 * stored["f32_minus_f64"]
    print("geometry LM: offset error %.3e -> %.3e in %d iterations (Adam: %.3e in %d); |f32 - f64| %.3e"
          % (stored["initial_error64"], stored["final_error64"], stored["iters"], RR.load_refine()["final_error64"],
             RR.load_refine()["K"], stored["f32_minus_f64"]))


def test_stored_gauss_newton_matches_a_fresh_run():
    """gauss_newton.json: the CG loop with the recorded cg_iters ends below a tenth of its initial loss after 3 LM steps, in
    float64 and in float32, both take the same accept / reject sequence, and the stored losses are reproduced.  The margin
    over the tenth is small (a gain of 11.1 against the required 10), so the gain is stored and held to 1e-3: a drift of the
    fixture shows here before it reaches the bound."""
    stored, fresh = R.load_gauss_newton(), R.measure_gauss_newton()
    assert (stored["steps"], stored["damping"], stored["cg_iters"]) == (R.GN_STEPS, R.GN_DAMPING, R.GN_CG_ITERS)
    assert stored["steps"] == 3 and (stored["sigma"], stored["seed"]) == (0.03, 3)
    assert stored["max_log_step"] == R.GN_MAX_LOG_STEP
    assert stored["gain64"] == stored["loss64"][0] / stored["loss64"][-1] and stored["gain64"] > 10.0 and stored["gain32"] > 10.0
    assert abs(fresh["gain64"] - stored["gain64"]) <= 1e-3 * stored["gain64"]
    assert abs(fresh["gain32"] - stored["gain32"]) <= 1e-3 * stored["gain32"]
    assert stored["loss64"][-1] < 0.1 * stored["loss64"][0] and stored["loss32"][-1] < 0.1 * stored["loss32"][0]
    assert stored["accepts64"] == stored["accepts32"] == fresh["accepts64"] == fresh["accepts32"]
    assert np.allclose(stored["loss64"], fresh["loss64"], rtol=1e-6, atol=0)
    assert 0.5 * stored["f32_minus_f64"] <= fresh["f32_minus_f64"] <= 2.0 * stored["f32_minus_f64"]
    print("cloud LM: loss %s, float32 %s, exact solves %s; |f32 - f64| %.3e" % (stored["loss64"], stored["loss32"],
                                                                                stored["loss64_exact_solves"], stored["f32_minus_f64"]))


def test_cg_solves_a_small_system():
    """cg_solve on a 5 x 5 symmetric positive definite system: exact after 5 iterations, and a singular direction with a zero
    preconditioner entry stays at 0."""
    g = np.random.RandomState(2)
    B = g.randn(8, 5)
    A = B.T @ B
    b = g.randn(5)
    x = R.cg_solve(lambda t: A @ t, b, 1.0 / np.diag(A), 5)
    assert np.allclose(A @ x, b, atol=1e-9)
    A[4, :] = A[:, 4] = 0.0
    b[4] = 0.0
    minv = np.where(np.diag(A) > 0, 1.0 / np.where(np.diag(A) > 0, np.diag(A), 1.0), 0.0)
    x = R.cg_solve(lambda t: A @ t, b, minv, 4)
    assert x[4] == 0.0 and np.allclose((A @ x)[:4], b[:4], atol=1e-9)
