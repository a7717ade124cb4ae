"""CPU: the restatement of the exact projector's ray gradient (tests/gaussian_project_rays_ref.py) against autograd, the
measured float32 error and host refinement loops the GPU tolerances are taken from, and r2_gaussian_amd.geometry.scan_rays
against scene.make_view and gradcheck."""
import os
import re

import numpy as np
import pytest
import torch

from tests import gaussian_project_rays_ref as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_stored_e32_matches_a_fresh_measurement():
    """tests/golden/gaussian_project_rays/e32.json (python -m tests.gaussian_project_rays_ref) within 10 % of a fresh one."""
    stored = Q.load_e32()
    assert sorted(stored) == sorted(Q.SCENES)
    for name in Q.SCENES:
        fresh = Q.measure_e32(name)
        assert abs(stored[name] - fresh) <= 0.1 * fresh, (name, stored[name], fresh)


@pytest.mark.parametrize("name", ["cone_p7", "parallel_p7", "cone_contains"])
def test_analytic_ray_gradient_matches_autograd(name):
    """The contract's per-pair formulas for g_s and g_d, summed into the twelve numbers per view, against torch.autograd
    through gaussian_project_ref.contract (float64): within 1e-10 of the sum of |contributions| (4e-14 measured)."""
    r = Q.reference(name)
    sc = r["scene"]
    auto = Q.torch_ray_grad(sc["rays"], sc["cone"], sc["H"], sc["W"], *sc["cloud"], sc["mod"], sc["G"])
    err = np.abs(auto - r["hi"]["grad"])
    print("%s: worst |autograd - analytic| / sum|contrib| = %.3e" % (name, (err / r["hi"]["gabs"]).max()))
    assert (r["hi"]["gabs"] > 0).all() and (err <= 1e-10 * r["hi"]["gabs"]).all()


def test_stored_refinement_matches_a_fresh_run():
    """tests/golden/gaussian_project_rays/refine.json: K and lr are the module's, the float64 loop ends below half its
    initial offset error (so the GPU test cannot pass by standing still), its final parameters are reproduced, and the
    float32 loop's distance from it -- the GPU test's tolerance is 4 x the stored one -- is reproduced within a factor 2."""
    stored, fresh = Q.load_refine(), Q.measure_refine()
    assert (stored["K"], stored["lr"]) == (Q.REFINE_K, Q.REFINE_LR)
    assert stored["final_error64"] < 0.5 * stored["initial_error64"]
    assert np.allclose(stored["final64"], fresh["final64"], rtol=0, atol=1e-9)
    assert 0.5 * stored["f32_minus_f64"] <= fresh["f32_minus_f64"] <= 2.0 * stored["f32_minus_f64"]


@pytest.mark.parametrize("beam", ["cone", "parallel"])
def test_scan_rays_restates_make_view(beam):
    """scan_rays at nominal values against world_ray_params([make_view(angle)]), three angles per beam.

    Bound: make_view stores the world-to-view matrix in float32 and world_ray_params derives the rays from it in float64 and
    rounds them to float32; scan_rays is float64 throughout.  With u = 2^-24: every rotation entry (|.| <= 1) carries at
    most u, so the axes ex, ey, ez read back from the inverse carry at most 3 u per entry (|R^T E R^T|_ij <= |E|_max
    sum_k |R_ki| sum_l |R_jl| <= 3 u); every translation entry (|.| <= DSO) carries at most u DSO, and the source position
    -t R^-1 then at most sqrt(3) u DSO + sqrt(3) DSO 3 u < 7 u DSO.  p00 adds the axes times factors of magnitude at most
    tan(fov / 2) <= 1, 1 and 1: at most 9 u.  The final rounding to float32 is at most u (DSO + 3).  Together
    u (8 DSO + 12) <= 10 u max(DSO, DSD) whenever max(DSO, DSD) >= 6, as here (DSO 5, DSD 7: 52 u against 70 u)."""
    from r2_gaussian_amd import geometry, scene as S
    from r2_gaussian_amd.gaussian_projector import world_ray_params
    scanner = dict(S.CONE_BEAM, mode=beam)
    DSO, DSD = scanner["DSO"], scanner["DSD"]
    assert max(scanner["sVoxel"]) == 2.0 and max(DSO, DSD) >= 6.0 and max(scanner["sDetector"]) / 2 <= DSD
    bound = 10.0 * 2.0 ** -24 * max(DSO, DSD)
    angles = [0.3, 2.4, 4.5]
    det = (17, 23)
    want = world_ray_params([S.make_view(a, det, scanner) for a in angles]).astype(np.float64)
    got = geometry.scan_rays(torch.tensor(angles, dtype=torch.float64), **geometry.scanner_args(scanner, det))
    assert got.dtype == torch.float64 and tuple(got.shape) == (3, 12)
    err = np.abs(got.numpy() - want).max()
    print("%s: max |scan_rays - world_ray_params| = %.3e, bound %.3e" % (beam, err, bound))
    assert err <= bound


def test_scan_rays_arguments_broadcast_and_move_the_detector():
    """Per-view tensors and scalars mix; offDetector moves p00 along the detector's own axes by that length over DSD (cone)
    and leaves the source alone; a roll of pi / 2 turns pu into pv's direction; d_angle adds to the angles."""
    from r2_gaussian_amd import geometry, scene as S
    kw = geometry.scanner_args(S.CONE_BEAM, (8, 12))
    ang = torch.tensor([0.1, 1.7], dtype=torch.float64)
    base = geometry.scan_rays(ang, **kw)
    off = geometry.scan_rays(ang, **dict(kw, offDetector=(torch.tensor([0.2, -0.1], dtype=torch.float64), 0.3)))
    unit = lambda t: t / t.norm(dim=1, keepdim=True)
    assert torch.equal(off[:, 0:3], base[:, 0:3]) and torch.equal(off[:, 6:12], base[:, 6:12])
    want = (0.3 * unit(base[:, 6:9]) + torch.tensor([[0.2], [-0.1]], dtype=torch.float64) * unit(base[:, 9:12])) / kw["DSD"]
    # float64 on coordinates of magnitude < 8: a few dozen roundings of at most 2^-53 * 8 = 9e-16 each
    assert torch.allclose(off[:, 3:6] - base[:, 3:6], want, rtol=0, atol=1e-13)
    rolled = geometry.scan_rays(ang, **dict(kw, roll=np.pi / 2))
    assert torch.allclose(unit(rolled[:, 6:9]), unit(base[:, 9:12]), rtol=0, atol=1e-13)
    assert torch.allclose(geometry.scan_rays(ang - 0.05, **kw, d_angle=0.05), base, rtol=0, atol=1e-13)
    with pytest.raises(ValueError):
        geometry.scan_rays(ang, **dict(kw, mode="fan"))
    with pytest.raises(ValueError):
        geometry.scan_rays(ang, **dict(kw, roll=torch.zeros(3)))


@pytest.mark.parametrize("beam", ["cone", "parallel"])
def test_scan_rays_gradcheck(beam):
    from r2_gaussian_amd import geometry
    g = torch.Generator().manual_seed(3)
    leaf = lambda *shape, at=0.0, by=0.1: (at + by * torch.randn(*shape, generator=g, dtype=torch.float64)).requires_grad_(True)
    angles, d_angle, DSO, DSD = leaf(3, at=1.0, by=1.0), leaf(3), leaf(1, at=5.0), leaf(3, at=7.0)
    dDet, offDet, roll, tilt, org = leaf(2, at=0.2, by=0.01), leaf(3, 2), leaf(3), leaf(2), leaf(3, 3)

    def f(angles, d_angle, DSO, DSD, dDet, offDet, roll, tilt, org):
        return geometry.scan_rays(angles, DSO, DSD, dDet, (5, 7), offDet, roll, tilt, org, beam, d_angle)

    assert torch.autograd.gradcheck(f, (angles, d_angle, DSO, DSD, dDet, offDet, roll, tilt, org), eps=1e-6, atol=1e-7, rtol=1e-6)


def test_symbols_are_declared():
    from r2_gaussian_amd import _lib
    with open(os.path.join(ROOT, "include", "r2hip.h")) as f:
        header = f.read()
    for name in ("r2_project_gaussians_rays_backward_workspace_bytes", "r2_project_gaussians_rays_backward"):
        assert re.search(r"R2_API\s+\w+\s+%s\(" % name, header), name
        assert name in _lib.exported_symbols()
    assert "#define R2_ABI_VERSION 3" in header or re.search(r"R2_ABI_VERSION\s+3\b", header)
