"""CPU: the restatement of the exact field query's contract (tests/gaussian_field_ref.py) against a plain expression and
autograd, the measured float32 error the GPU tolerance is taken from, the sphere that makes "q <= 32 is always summed" true,
the voxel positions, the bracket that prices the voxelizer's cut, and the Morton order."""
import numpy as np
import pytest
import torch

from tests import gaussian_field_ref as R


def _f64(sc):
    return [torch.from_numpy(np.asarray(a, np.float64)) for a in sc["cloud"]], torch.from_numpy(sc["points"].reshape(-1, 3).astype(np.float64))


def _plain(points, xyz, density, scaling, rotation, mod=1.0):
    """sum_i rho_i exp(-(x - mu_i)^T A_i (x - mu_i) / 2) with A = R S^-2 R^T by matrix products: the contract's q = |S^-1 R^T e|^2.
    A is Sigma^-1 = (R S^2 R^T)^-1 when the quaternion has norm 1; for a raw quaternion R is not orthogonal and the contract
    (like r2_project_gaussians') means A."""
    r, x, y, z = rotation.unbind(1)
    Rm = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
                      2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                      2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], 1).reshape(-1, 3, 3)
    A = Rm @ torch.diag_embed((scaling * mod) ** -2) @ Rm.transpose(1, 2)
    e = points[:, None, :] - xyz[None, :, :]
    q = torch.einsum("npi,pij,npj->np", e, A, e)
    return (density.reshape(1, -1) * torch.exp(-0.5 * q)).sum(1)


@pytest.mark.parametrize("name", ["plane", "raw_quat", "mod_half", "offset"])
def test_field64_is_the_plain_expression(name):
    sc = R.reference(name)["scene"]
    cloud, pts = _f64(sc)
    want = _plain(pts, *cloud, mod=sc["mod"]).numpy()
    got = R.reference(name)["hi"]
    assert (np.abs(got["val"] - want) <= 1e-9 * got["abs"] + 1e-300).all()


def test_analytic_gradients_match_autograd():
    """The contract's per-pair gradient formulas, summed, against torch.autograd through the same restatement (float64), for
    all five gradients."""
    sc = R.reference("raw_quat")["scene"]
    ana = R.reference("raw_quat")["hi"]
    cloud, pts = _f64(sc)
    leaves = [t.requires_grad_(True) for t in cloud + [pts]]
    val = R.torch_field(leaves[4], *leaves[:4], mod=sc["mod"])
    assert np.allclose(val.detach().numpy(), ana["val"], rtol=1e-12, atol=0)
    (val * torch.from_numpy(sc["G"].astype(np.float64))).sum().backward()
    for k, t in zip(R.GRADS, leaves):
        err = np.abs(t.grad.numpy().reshape(ana["grads"][k].shape) - ana["grads"][k])
        assert (err <= 1e-10 * ana["gabs"][k] + 1e-300).all(), k


def test_gradcheck_of_the_restatement():
    sc = R.scene("tail_1")
    cloud = [torch.from_numpy(a[:3].astype(np.float64)).requires_grad_(True) for a in sc["cloud"]]
    pts = (cloud[0].detach()[[0, 1, 2, 0]] + torch.tensor([[0.05, -0.02, 0.03], [0.0, 0.04, -0.06], [-0.03, 0.01, 0.02],
                                                          [0.2, 0.1, -0.1]], dtype=torch.float64)).requires_grad_(True)
    f = lambda p, x, d, s, r: R.torch_field(p, x, d, s, r, 0.8)
    assert torch.autograd.gradcheck(f, [pts] + cloud, eps=1e-7, atol=1e-6, rtol=1e-5)


def test_stored_e32_matches_a_fresh_measurement():
    """tests/golden/gaussian_field/e32.json (python -m tests.gaussian_field_ref) within 10 % of a fresh measurement, the
    tolerance tests/test_gaussian_project_cpu.py uses for the projector's file."""
    stored = R.load_e32()
    assert sorted(stored) == sorted(R.SCENES)
    for name in R.SCENES:
        fresh = R.measure_e32(name)
        assert sorted(fresh) == sorted(stored[name])
        for k, v in fresh.items():
            assert abs(stored[name][k] - v) <= 0.1 * v, (name, k, stored[name][k], v)


@pytest.mark.parametrize("name", R.SCENES)
def test_pairs_with_q_up_to_32_lie_inside_the_sphere(name):
    """The "always summed" rule: every pair with q <= 32 (float64) has |x - mu| <= radius / 1.009 for the shared sphere
    (gauss_radius: 1.01 sqrt(32) sigma_max / s_min(R)), so the 1 % is there in full for float32 to spend; on raw_quat this
    holds only with the closed form of s_min."""
    sc = R.reference(name)["scene"]
    xyz, dens, scal, rot = sc["cloud"]
    if xyz.shape[0] == 0:
        return
    pts = sc["points"].reshape(-1, 3).astype(np.float64)
    x = [pts[:, j:j + 1] for j in range(3)]
    cols = lambda a: R._cols(a, np.float64)
    with np.errstate(all="ignore"):
        o = R.contract(np, x, cols(xyz), cols(dens.reshape(-1, 1))[0], cols(scal), np.float64(sc["mod"]), cols(rot), qmax=32.0)
        dist = np.sqrt(o["e"][0] ** 2 + o["e"][1] ** 2 + o["e"][2] ** 2)
        radius = R.sphere_radius(scal, rot, sc["mod"])[None, :]
        inside = dist <= radius / 1.009
    assert inside[o["keep"]].all()
    if name in ("plane", "raw_quat", "tiny"):
        assert o["keep"].sum() > 100   # the check is not vacuous


def test_voxel_centres_are_the_voxelizers(oracle):
    """The oracle voxelizer puts the mean m at (m - center + sVoxel / 2) / dVoxel in voxel units and samples voxel idx at
    idx + 0.5: a Gaussian placed at voxel_centres[idx] lands there (float32: within 1e-5 voxels of it)."""
    from r2_gaussian_amd.field import voxel_centres
    center, n, s = (0.2, -0.1, 0.3), (5, 7, 6), (0.25, 0.5, 0.3)
    vc = voxel_centres(center, n, s)
    assert vc.shape == (5, 7, 6, 3) and vc.dtype == torch.float32
    assert np.array_equal(vc.numpy(), R.patch_centres(center, n, s))
    means = vc.reshape(-1, 3).numpy()
    P = means.shape[0]
    rot = np.tile(np.array([[1.0, 0.0, 0.0, 0.0]], np.float32), (P, 1))
    st = oracle.voxel_forward(means, np.ones((P, 1), np.float32), np.full((P, 3), 0.05, np.float32), rot, 1.0, None, n, s, center,
                              render=False)
    idx = np.stack(np.meshgrid(*[np.arange(k) for k in n], indexing="ij"), -1).reshape(-1, 3)
    assert (st["radii_x"] > 0).all()
    assert np.abs(st["means3D_norm"] - (idx + 0.5)).max() <= 1e-5


def test_oracle_voxelizer_lies_in_the_field_bracket(oracle):
    """The voxelizer's cut, priced: the oracle's volume of the 16^3 grid of 150 Gaussians lies between the field's pairs with
    q <= 9 and term >= 2e-6 and the field itself (tests/gaussian_field_ref.voxel_bracket has the derivation), at every
    voxel."""
    b = R.voxel_bracket()
    st = oracle.voxel_forward(*b["cloud"], 1.0, None, b["nVoxel"], b["sVoxel"], b["center"])
    vol = st["vol"].astype(np.float64)
    assert np.array_equal(st["vol"], np.load(R.VOXEL_GOLDEN)["fw_vol"])
    print("oracle voxelizer: min (vol - lo) %.3e, min (hi - vol) %.3e, max (hi - lo) / max(vol) %.3e"
          % ((vol - b["lo"]).min(), (b["hi"] - vol).min(), (b["hi"] - b["lo"]).max() / vol.max()))
    assert (vol >= b["lo"]).all() and (vol <= b["hi"]).all()
    assert (b["hi"] - b["lo"]).max() > 1e-3 * vol.max()   # the cut is visible: the bracket is not a tolerance band


def test_morton_order_is_a_stable_permutation():
    from r2_gaussian_amd.field import inverse_permutation, morton_order
    pts = torch.from_numpy(R.scene("scattered")["points"]).clone()
    pts[3, 0], pts[10, 2] = float("nan"), float("inf")
    perm = morton_order(pts)
    N = pts.shape[0]
    assert perm.dtype == torch.int64 and torch.equal(torch.sort(perm)[0], torch.arange(N))
    inv = inverse_permutation(perm)
    assert torch.equal(perm[inv], torch.arange(N)) and torch.equal(inv[perm], torch.arange(N))
    assert torch.equal(pts[perm][inv].nan_to_num(7.0, 8.0, 9.0), pts.nan_to_num(7.0, 8.0, 9.0))
    # coherent: the mean distance between neighbours in the sorted order is far below that of the given (random) order
    fin = torch.isfinite(pts).all(1)
    step = lambda p: (p[1:] - p[:-1]).norm(dim=1).mean()
    assert step(pts[perm][fin[perm]]) < 0.5 * step(pts[fin])
    # equal keys keep their order; no points, one point, coincident points
    same = torch.zeros((5, 3))
    assert torch.equal(morton_order(same), torch.arange(5))
    assert morton_order(torch.zeros((0, 3))).shape == (0,) and torch.equal(morton_order(torch.ones((1, 3))), torch.arange(1))
