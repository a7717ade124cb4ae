"""CPU: the restatement of the contract of the exact line integrals along caller-supplied rays (tests/gaussian_bundle_ref.py)
against autograd and against the projector's own restatement, the measured float32 error the GPU tolerance is taken from, the
ray generators of r2_gaussian_amd.geometry, and the sort key."""
import numpy as np
import pytest
import torch

from tests import gaussian_bundle_ref as B
from tests import gaussian_project_ref as R


def test_stored_e32_matches_a_fresh_measurement():
    """tests/golden/gaussian_bundle/e32.json (python -m tests.gaussian_bundle_ref) within 10 % of a fresh measurement, the
    tolerance tests/test_gaussian_field_cpu.py uses for the field's file."""
    stored = B.load_e32()
    assert sorted(stored) == sorted(B.SCENES)
    for name in B.SCENES:
        fresh = B.measure_e32(name)
        assert sorted(fresh) == sorted(stored[name])
        for k, v in fresh.items():
            assert abs(stored[name][k] - v) <= 0.1 * v, (name, k, stored[name][k], v)


@pytest.mark.parametrize("name", ["raw_quat", "inside"])
def test_analytic_gradients_match_autograd(name):
    """The per-pair gradient formulas, summed, against torch.autograd through the same pair (float64), for the four parameter
    gradients and both ray gradients; `inside` has the cone rule in force."""
    sc, ana = B.reference(name)["scene"], B.reference(name)["hi"]
    f64 = lambda a: torch.from_numpy(np.asarray(a, np.float64)).requires_grad_(True)
    cloud = [f64(a) for a in sc["cloud"]]
    o, d = f64(sc["origins"].reshape(-1, 3)), f64(sc["directions"].reshape(-1, 3))
    val = B.torch_bundle(o, d, sc["half_line"], *cloud, mod=sc["mod"])
    assert np.allclose(val.detach().numpy(), ana["val"], rtol=1e-12, atol=0)
    (val * torch.from_numpy(sc["G"].astype(np.float64))).sum().backward()
    for k, t in zip(B.GRADS, cloud + [o, d]):
        err = np.abs(t.grad.numpy().reshape(ana["grads"][k].shape) - ana["grads"][k])
        assert (err <= 1e-9 * ana["gabs"][k] + 1e-300).all(), k
    if name == "inside":   # the cone rule bites: a good part of the pairs, not all
        s = [o.detach().numpy()[:, j:j + 1] for j in range(3)]
        dd = [d.detach().numpy()[:, j:j + 1] for j in range(3)]
        cols = lambda a: R._cols(a, np.float64)
        xyz, dens, scal, rot = sc["cloud"]
        kept = [R.contract(np, s, dd, h, cols(xyz), cols(dens)[0], cols(scal), 1.0, cols(rot), qmax=32.0)["keep"].sum() for h in (True, False)]
        assert 0.2 * kept[1] < kept[0] < 0.8 * kept[1]


@pytest.mark.parametrize("beam", ["cone", "parallel"])
def test_flat_bundle_is_the_projectors_image(beam):
    """On the pixel rays of a flat detector the float64 bundle is gaussian_project_ref's image and parameter gradients, pair
    for pair (the same pairs of the same float64 rays, summed in another order), for q <= 32 and for every pair; the scene's
    float32 rays are the projector's, bit for bit."""
    sc = B.reference("flat_" + beam)["scene"]
    ps = R.reference(beam + "_p300_small")
    pr = ps["scene"]
    S, D = R.pixel_rays(pr["rays"], pr["cone"], pr["H"], pr["W"], np.float32)
    assert np.array_equal(np.stack(S, -1).reshape(-1, 3), sc["origins"].reshape(-1, 3))
    assert np.array_equal(np.stack(D, -1).reshape(-1, 3), sc["directions"].reshape(-1, 3))
    assert np.array_equal(sc["G"], pr["G"].reshape(-1)) and sc["half_line"] == pr["cone"]
    S, D = R.pixel_rays(pr["rays"], pr["cone"], pr["H"], pr["W"], np.float64)
    for which, qmax in (("lo", 32.0), ("hi", None)):
        a = B.bundle64(np.stack(S, -1), np.stack(D, -1), sc["half_line"], *sc["cloud"], mod=sc["mod"], qmax=qmax, G=sc["G"])
        b = ps[which]
        assert (np.abs(a["val"] - b["img"].reshape(-1)) <= 1e-13 * b["abs"].reshape(-1) + 1e-300).all()
        for k in B.PARAMS:
            assert (np.abs(a["grads"][k] - b["grads"][k]) <= 1e-12 * b["gabs"][k] + 1e-300).all(), (which, k)


def test_pixel_rays():
    """The whole detector, chosen pixels per view, the same pixels in every view; gradients reach the [V,12] rays."""
    from r2_gaussian_amd import geometry
    pr = R.scene("cone_p7")
    rays, H, W = torch.from_numpy(pr["rays"]), pr["H"], pr["W"]
    for cone in (True, False):
        o, d = geometry.pixel_rays(rays, cone, H, W)
        assert o.shape == d.shape == (3, H, W, 3) and o.dtype == torch.float32
        S, D = R.pixel_rays(pr["rays"], cone, H, W, np.float32)
        assert np.array_equal(o.numpy(), np.stack(S, -1)) and np.array_equal(d.numpy(), np.stack(D, -1))
        g = torch.Generator().manual_seed(3)
        rows, cols = torch.randint(H, (3, 11), generator=g), torch.randint(W, (3, 11), generator=g)
        o2, d2 = geometry.pixel_rays(rays, cone, H, W, rows, cols)
        v = torch.arange(3)[:, None]
        assert torch.equal(o2, o[v, rows, cols]) and torch.equal(d2, d[v, rows, cols])
        o3, d3 = geometry.pixel_rays(rays, cone, H, W, rows[:1], cols[:1])
        assert o3.shape == (3, 11, 3) and torch.equal(d3, d[:, rows[0], cols[0]]) and torch.equal(o3, o[:, rows[0], cols[0]])
    r64 = rays.double().requires_grad_(True)
    o, d = geometry.pixel_rays(r64, True, H, W)
    (o.sum() + 2.0 * d.sum()).backward()
    want = torch.zeros(12, dtype=torch.float64)
    c, r = sum(range(W)) * H, sum(range(H)) * W
    want[0:3], want[3:6], want[6:9], want[9:12] = H * W - 2.0 * H * W, 2.0 * H * W, 2.0 * c, 2.0 * r
    assert torch.allclose(r64.grad, want.expand(3, 12), rtol=1e-12)
    with pytest.raises(ValueError):
        geometry.pixel_rays(rays[:, :11], True, H, W)
    with pytest.raises(ValueError):
        geometry.pixel_rays(rays, True, H, W, rows=torch.zeros((3, 2), dtype=torch.int64))
    with pytest.raises(ValueError):
        geometry.pixel_rays(rays, True, H, W, torch.zeros((2, 2), dtype=torch.int64), torch.zeros((2, 2), dtype=torch.int64))
    with pytest.raises(ValueError):
        geometry.pixel_rays(rays, True, 0, W)


def test_curved_detector_rays():
    """Every ray starts at the source; every pixel lies on the cylinder of radius DSD about the source's axis, at equal
    angles; on the central column the rays are those of scan_rays' flat detector with the same row pitch through pixel_rays;
    differentiable in its continuous arguments."""
    from r2_gaussian_amd import geometry
    angles = torch.tensor([0.3, 2.4, 4.0], dtype=torch.float64)
    DSO, DSD, dG, dV, H, W = 5.0, 7.0, 0.012, 0.09, 9, 31
    o, d = geometry.curved_detector_rays(angles, DSO, DSD, dG, dV, (H, W))
    assert o.shape == d.shape == (3, H, W, 3) and o.dtype == torch.float64
    src = DSO * torch.stack([angles.cos(), angles.sin(), torch.zeros(3, dtype=torch.float64)], 1)
    assert torch.allclose(o, src[:, None, None, :].expand_as(o), rtol=0, atol=1e-15)
    pix = o + DSD * d
    assert torch.allclose((pix - o)[..., :2].norm(dim=-1), torch.full((3, H, W), DSD, dtype=torch.float64), rtol=1e-14)
    en = -src / DSO
    fan = torch.atan2(d[..., 0] * en[:, None, None, 1] - d[..., 1] * en[:, None, None, 0],
                      d[..., 0] * en[:, None, None, 0] + d[..., 1] * en[:, None, None, 1])
    assert torch.allclose((fan[:, :, 1:] - fan[:, :, :-1]).abs(), torch.full((3, H, W - 1), dG, dtype=torch.float64), rtol=1e-9)
    flat = geometry.scan_rays(angles, DSO, DSD, (dV, 0.05), (H, W))
    fo, fd = geometry.pixel_rays(flat, True, H, W)
    mid = (W - 1) // 2
    assert torch.allclose(o[:, :, mid], fo[:, :, mid], rtol=0, atol=1e-14) and torch.allclose(d[:, :, mid], fd[:, :, mid], rtol=0, atol=1e-14)
    # the offsets: along the rows a length, along the arc DSD times an angle (one column further: one dGamma)
    o2, d2 = geometry.curved_detector_rays(angles, DSO, DSD, dG, dV, (H, W), offDetector=(dV, DSD * dG))
    assert torch.allclose(d2[:, :-1, :-1], d[:, 1:, 1:], rtol=0, atol=1e-14)
    a = angles.clone().requires_grad_(True)
    dso = torch.tensor(DSO, dtype=torch.float64, requires_grad=True)
    f = lambda a, s, g: torch.cat(geometry.curved_detector_rays(a, s, DSD, g, dV, (2, 3)), -1)
    assert torch.autograd.gradcheck(f, [a, dso, torch.tensor(dG, dtype=torch.float64, requires_grad=True)], eps=1e-6, atol=1e-7)
    with pytest.raises(ValueError):
        geometry.curved_detector_rays(angles, DSO, DSD, dG, dV, (0, 3))


def test_ray_order_is_a_stable_permutation_that_groups_rays():
    from r2_gaussian_amd.gaussian_projector import ray_order
    sc = B.scene("scattered")
    o, d = torch.from_numpy(sc["origins"]).clone(), torch.from_numpy(sc["directions"]).clone()
    o[3, 0], d[10, 2], d[11] = float("nan"), float("inf"), 0.0
    xyz = torch.from_numpy(sc["cloud"][0])
    perm = ray_order(o, d, xyz)
    N = o.shape[0]
    assert perm.dtype == torch.int64 and torch.equal(torch.sort(perm)[0], torch.arange(N))
    # coherent: neighbours in the order pass the cloud's centre far closer to each other than neighbours in the given order
    h = torch.nn.functional.normalize(d.double(), dim=1)
    near = o.double() - (o.double() * h).sum(1, keepdim=True) * h
    fin = torch.isfinite(near).all(1)
    step = lambda p: (p[1:] - p[:-1]).norm(dim=1).mean()
    assert step(near[perm][fin[perm]]) < 0.6 * step(near[fin])
    same = torch.zeros((5, 3))
    assert torch.equal(ray_order(same, same + 1.0, xyz), torch.arange(5))
    assert ray_order(o[:0], d[:0], xyz).shape == (0,) and torch.equal(ray_order(o, d, xyz[:0]), torch.arange(N))
