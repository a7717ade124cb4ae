"""CPU: the float64 restatement of the iterative reconstructions (tests/recon_ref.py) against first principles -- CGLS
reaches the least-squares solution, SART a solution of a consistent system, grad TV_eps matches finite differences, ASD-POCS
ends with less TV than SART -- and recon.py's host-side validation, which raises before anything reaches a GPU."""
import numpy as np
import pytest

from r2_gaussian_amd import _lib
from r2_gaussian_amd import fdk as F
from r2_gaussian_amd import recon as RC
from r2_gaussian_amd import scene as S
from tests import recon_ref as RR


def test_cgls_converges_to_lstsq():
    rng = np.random.RandomState(0)
    A = rng.rand(40, 12)
    b = rng.rand(40)
    xs, l2 = RR.cgls(A, b, 30)
    want = np.linalg.lstsq(A, b, rcond=None)[0]
    assert np.allclose(xs[-1], want, rtol=1e-9, atol=1e-9)
    assert all(l2[i + 1] <= l2[i] * (1 + 1e-12) for i in range(len(l2) - 1))


def test_sart_fixed_point_on_a_consistent_system():
    rng = np.random.RandomState(1)
    A = rng.rand(36, 9) * (rng.rand(36, 9) < 0.6)
    truth = rng.rand(9) + 0.1
    b = A @ truth
    for bs in (1, 3, 12):
        x = RR.ossart(A, b, 3, 3000, bs, lmbda=1.0, lmbda_red=1.0)[-1]
        assert np.linalg.norm(A @ x - b) <= 1e-6 * np.linalg.norm(b), bs
        # a solution stays put
        again = RR.ossart(A, b, 3, 1, bs, 1.0, 1.0, x0=truth)[-1]
        assert np.allclose(again, truth, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("shape", [(5, 4, 6), (1, 1, 7), (1, 5, 4), (2, 2, 2)])
def test_tv_gradient_against_finite_differences(shape):
    rng = np.random.RandomState(sum(shape))
    x = rng.rand(*shape)
    g = RR.tv_grad(x)
    h = 1e-6
    fd = np.zeros_like(x)
    for idx in np.ndindex(*shape):
        e = np.zeros_like(x)
        e[idx] = h
        fd[idx] = (RR.tv_value(x + e) - RR.tv_value(x - e)) / (2 * h)
    assert np.allclose(g, fd, rtol=1e-5, atol=1e-6)
    # a constant volume has a zero gradient and descent leaves it alone
    c = np.full(shape, 0.3)
    assert not RR.tv_grad(c).any()
    assert np.array_equal(RR.tv_descent(c, 0.1, 3), c)


def _tiny_cfg(n=6, det=(9, 9), mode="cone"):
    base = S.CONE_BEAM if mode == "cone" else S.PARALLEL_BEAM
    return dict(base, nVoxel=[n, n, n], nDetector=list(det), sVoxel=[2.0, 2.0, 2.0], offOrigin=[0.0, 0.0, 0.0],
                sDetector=[3.2, 3.2], accuracy=0.5, filter=None)


def test_asd_pocs_ends_with_less_tv_than_sart():
    cfg = _tiny_cfg()
    angles = np.linspace(0, 2 * np.pi, 13)[:-1] + 0.05
    A, bd = RR.dense_A_cfg(cfg, angles)
    n = 6
    ax = (np.arange(n) + 0.5) / n * 2 - 1
    X, Y, Z = np.meshgrid(ax, ax, ax, indexing="ij")
    truth = ((X ** 2 + Y ** 2 + Z ** 2) < 0.5).astype(np.float64) * 0.8
    rng = np.random.RandomState(2)
    b = A @ truth.ravel()
    b = b + rng.normal(0, 0.05 * b.max(), b.shape) * (b > 0)
    rows = 81
    x_sart = RR.ossart(A, b, rows, 10, 1, 1.0, 0.9999)[-1]
    x_asd, tr = RR.os_asd_pocs(A, b, (n, n, n), rows, 10, 1, maxl2err=0.0, alpha=0.2)
    assert RR.tv_value(x_asd.reshape(n, n, n)) < RR.tv_value(x_sart.reshape(n, n, n))
    assert all(v >= 0 for xs in tr["x_sart"] for v in xs)


def test_dense_A_is_the_projection():
    """A x from the dense matrix equals projector_ref's projection of x (linearity of the restatement)."""
    from tests import projector_ref as PR
    from r2_gaussian_amd import projector as K
    cfg = _tiny_cfg(n=4, det=(6, 7), mode="parallel")
    angles = [0.3, 1.9]
    A, _ = RR.dense_A_cfg(cfg, angles)
    views, sV, ctr, scale = RR.scene_geometry(cfg, angles)
    x = np.random.RandomState(3).rand(4, 4, 4)
    r = PR.project(x, K.ray_params(views, sV, ctr, (4, 4, 4)), False, np.asarray(sV) / 4, 0.5, 6, 7)
    assert np.allclose(A @ x.ravel(), r["value"] / scale, rtol=1e-12, atol=1e-14)


def test_host_side_validation():
    cfg = _tiny_cfg()
    with pytest.raises(ValueError):
        RC.Operator([0.0], cfg, accuracy=0.0)
    with pytest.raises(ValueError):
        RC.Operator([], cfg)
    with pytest.raises(_lib.R2HipError):
        RC.Operator([0.0], cfg, device="cpu")
    with pytest.raises(ValueError):
        RC.recon_volume(np.zeros((1, 9, 9), np.float32), [0.0], cfg, "sart")
    with pytest.raises(ValueError):
        F.recon_volume(np.zeros((1, 9, 9), np.float32), [0.0], cfg, "sart")
    with pytest.raises(AssertionError):
        F.init_pcd(np.zeros((1, 9, 9), np.float32), [0.0], cfg, recon_method="cgls")
    import torch
    with pytest.raises(_lib.R2HipError):
        RC.tv_descent(torch.zeros(3, 3, 3), 0.1, 1)
    with pytest.raises(_lib.R2HipError):
        RC.backproject_views(torch.zeros(1, 4, 4), [S.make_view(0.0, (4, 4))], (2, 2, 2), (0, 0, 0), 0.5, nVoxel=(3, 3, 3))
    with pytest.raises(NotImplementedError):
        RC.reconstruct(np.zeros((1, 9, 9), np.float32), [0.0], cfg, "fista")
