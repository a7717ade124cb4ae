"""CPU: the restatement of the exact Gaussian projector's contract (tests/gaussian_project_ref.py) against quadrature and
autograd, the measured float32 error the GPU tolerance is taken from, and why the contract forbids the cancelling form of q."""
import json
import math

import numpy as np
import pytest
import torch

from tests import gaussian_project_ref as R


def _rot64(q):
    return np.array([[float(np.asarray(c)) for c in row] for row in R._rot([np.float64(v) for v in q])])


# three anisotropic rotated Gaussians: (mean, density, scales, quaternion)
GAUSSIANS = [((0.1, -0.2, 0.05), 0.7, (0.05, 0.3, 0.12), (0.9, 0.1, -0.3, 0.2)),
             ((-0.3, 0.1, 0.2), 1.3, (0.4, 0.02, 0.1), (0.3, -0.5, 0.6, 0.4)),
             ((0.0, 0.0, 0.0), 0.4, (0.01, 0.5, 0.07), (0.7, 0.0, 0.7, 0.1))]


def _quadrature(s, d, mu, rho, sig, q, nodes=400001):
    """Trapezoid rule for rho exp(-x^T Sigma^-1 x / 2) along s + t d over +-12 sigma around the closest approach."""
    Rm = _rot64(q)
    M = (Rm / np.asarray(sig)[None, :]).T            # S^-1 R^T
    u, w = M @ d, M @ (s - mu)
    ts = -(u @ w) / (u @ u)
    half = 12.0 / math.sqrt(u @ u)
    t = np.linspace(ts - half, ts + half, nodes)
    y = w[:, None] + u[:, None] * t[None, :]
    f = rho * np.exp(-0.5 * (y * y).sum(0))
    return float(((f[:-1] + f[1:]).sum() * 0.5) * (t[1] - t[0]) * np.linalg.norm(d))


@pytest.mark.parametrize("cone", [True, False])
@pytest.mark.parametrize("gi", [0, 1, 2])
def test_closed_form_matches_quadrature(cone, gi):
    mu, rho, sig, q = GAUSSIANS[gi]
    qn = np.asarray(q) / np.linalg.norm(q)
    Rm = _rot64(qn)
    src = np.array([5.0, 0.4, -0.3])
    # a ray towards the Gaussian, one passing at an angle, and one parallel to the principal axis R[:, 1]
    dirs = [np.asarray(mu) + np.array([0.02, -0.01, 0.03]) - src, np.array([-5.0, 0.1, 0.4]), Rm[:, 1] * (-1.0 if Rm[0, 1] > 0 else 1.0)]
    for k, dv in enumerate(dirs):
        if cone:
            s = src if k < 2 else np.asarray(mu) - 4.0 * dv + 0.5 * np.asarray(sig)[0] * Rm[:, 0]
        else:
            s = np.asarray(mu) + 0.7 * np.asarray(sig)[0] * Rm[:, 0] - 3.0 * dv
        col = lambda a: [np.array([[float(x)]]) for x in a]
        o = R.contract(np, col(s), col(dv), cone, col(mu), np.array([[rho]]), col(sig), 1.0, col(qn))
        ref = _quadrature(np.asarray(s, np.float64), np.asarray(dv, np.float64), np.asarray(mu), rho, sig, qn)
        got = float(o["term"][0, 0])
        assert bool(o["keep"][0, 0]) and ref > 0
        assert abs(got - ref) <= 1e-9 * ref, (k, got, ref)


@pytest.mark.parametrize("beam", ["cone", "parallel"])
def test_analytic_gradients_match_autograd(beam):
    """The contract's per-pair gradient formulas, summed, against torch.autograd through the same restatement (float64)."""
    sc = R.scene(beam + "_p7")
    H, W = 5, 6
    rays = sc["rays"][:2]
    G = np.random.RandomState(1).rand(2, H, W) * 2 - 1
    ana = R.project64(rays, sc["cone"], H, W, *sc["cloud"], G=G.astype(np.float32))
    leaves = [torch.from_numpy(a.astype(np.float64)).requires_grad_(True) for a in sc["cloud"]]
    img = R.torch_image(rays, sc["cone"], H, W, *leaves)
    assert np.allclose(img.detach().numpy(), ana["img"], rtol=1e-12, atol=0)
    (img * torch.from_numpy(G.astype(np.float32).astype(np.float64))).sum().backward()
    for k, t in zip(R.GRADS, leaves):
        err = np.abs(t.grad.numpy().reshape(ana["grads"][k].shape) - ana["grads"][k])
        assert (err <= 1e-10 * ana["gabs"][k] + 1e-300).all(), k


def test_gradcheck_of_the_restatement():
    sc = R.scene("cone_p7")
    leaves = [torch.from_numpy(a[:2].astype(np.float64)).requires_grad_(True) for a in sc["cloud"]]
    f = lambda x, d, s, r: R.torch_image(sc["rays"][:1], True, 3, 4, x, d, s, r)
    assert torch.autograd.gradcheck(f, leaves, eps=1e-7, atol=1e-6, rtol=1e-5)


def test_bounding_radius_contains_the_q32_ellipsoid():
    """csrc/gaussian_rays.hpp: |x| <= sqrt(32) sigma_max / s_min(R) on {x: |S^-1 R^T x|^2 <= 32}, with the closed form of
    s_min for a quaternion used as it comes, against the singular values of R."""
    g = np.random.RandomState(0)
    for _ in range(200):
        q = g.randn(4) * g.choice([0.3, 1.0, 2.0])
        n2 = float(q @ q)
        smin2 = min(1.0, (1 - n2) ** 2 + 2 * (1 - n2) * (2 * q[0] ** 2 - n2) + n2 ** 2)
        sv = np.linalg.svd(_rot64(q), compute_uv=False)
        assert abs(math.sqrt(max(smin2, 0.0)) - sv.min()) <= 1e-9 * max(1.0, sv.max())


def test_stored_e32_matches_a_fresh_measurement():
    """tests/golden/gaussian_project/e32.json (python -m tests.gaussian_project_ref) within 10 % of a fresh measurement."""
    stored = R.load_e32()
    assert sorted(stored) == sorted(R.SCENES)
    for name in R.SCENES:
        fresh = R.measure_e32(name)
        for k, v in fresh.items():
            assert abs(stored[name][k] - v) <= 0.1 * v, (name, k, stored[name][k], v)


@pytest.mark.parametrize("beam", ["cone", "parallel"])
def test_cancelling_form_loses_its_digits(beam):
    """q = w.w - B^2 / A in float32 on the small-sigma scene: more than 100 x the error of the contract's form."""
    name = beam + "_small_sigma"
    good, bad = R.measure_e32(name)["image"], R.measure_e32(name, cancelling=True)["image"]
    print("%s: e32 %.3e, cancelling form %.3e" % (name, good, bad))
    assert bad > 100.0 * good
