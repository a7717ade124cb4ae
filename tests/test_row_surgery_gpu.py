"""GPU: the row copy that densify_ops.hip and gaussian_mcmc.hip share (csrc/cloud_model.hpp: cloud_copy_row) at P = 1 and at
P = 257, one row past a 256-thread workgroup, with moments and statistics and without moments: surgery that changes nothing
returns every array bit for bit, and a relocation leaves every row it neither moves nor draws from bit for bit."""
import numpy as np
import pytest
import torch

from tests import mcmc_ref as R

pytestmark = pytest.mark.gpu


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and bool(torch.equal(_bits(a), _bits(b)))


def _rows(gpu, raw, P, with_moments):
    g = torch.Generator().manual_seed(P)
    p = {n: torch.from_numpy(raw[n]).to(gpu) for n in R.NAMES}
    moments = {n: (torch.randn(p[n].shape, generator=g).to(gpu), torch.rand(p[n].shape, generator=g).to(gpu))
               for n in R.NAMES} if with_moments else None
    stats = tuple((torch.rand(P, generator=g) + 0.5).to(gpu) for _ in range(3))
    return p, moments, stats


def _check_same(tag, p, moments, stats, new_p, new_m, new_s, rows=slice(None)):
    for n in R.NAMES:
        assert _same_bits(new_p[n][rows], p[n][rows]), tag + (n,)
        if moments is not None:
            assert _same_bits(new_m[n][0][rows], moments[n][0][rows]) and _same_bits(new_m[n][1][rows], moments[n][1][rows]), tag + (n,)
    assert (new_m is None) == (moments is None)
    if stats is not None:
        for k in range(3):
            assert _same_bits(new_s[k].reshape(-1)[rows], stats[k][rows]), tag + ("stat", k)


@pytest.mark.parametrize("with_moments", (True, False))
@pytest.mark.parametrize("P", (1, 257))
def test_a_prune_that_prunes_nothing_is_the_identity(gpu, P, with_moments):
    """do_densify=False, no density below -1, a bounding box that holds everything, no screen or scale threshold."""
    from r2_gaussian_amd import densify as D
    p, moments, stats = _rows(gpu, R.cloud(P, 40 + P), P, with_moments)
    normals = torch.randn((2, P, 3), generator=torch.Generator().manual_seed(1))
    bbox = torch.tensor([[-1e30] * 3, [1e30] * 3])
    new_p, new_m, mr, ga, dn, cnt = D.densify_and_prune(p, moments, *stats, normals, 0.0, 0.05, -1.0, bbox, do_densify=False)
    assert cnt == (P, 0, 0, 0)
    _check_same((P, with_moments), p, moments, stats, new_p, new_m, (mr, ga, dn))


@pytest.mark.parametrize("with_moments", (True, False))
@pytest.mark.parametrize("P", (1, 257))
def test_a_relocation_with_nothing_dead_and_nothing_new_is_the_identity(gpu, P, with_moments):
    """dead_density = -1 (an activated density is >= 0) and n_new = 0; without moments also without statistics."""
    from r2_gaussian_amd import mcmc as MC
    p, moments, stats = _rows(gpu, R.cloud(P, 40 + P), P, with_moments)
    stats = stats if with_moments else None
    new_p, new_m, new_s, info = MC.relocate(p, moments, stats, -1.0, n_new=0, seed=2, call=P, counts=True)
    assert (info["dead"], info["alive"], info["P"]) == (0, P, P)
    assert bool((info["sources"] == -1).all()) and bool((info["draws"] == 0).all())
    assert (new_s is None) == (stats is None)
    _check_same((P, with_moments), p, moments, stats, new_p, new_m, new_s)


@pytest.mark.parametrize("with_moments", (True, False))
def test_a_relocation_leaves_the_other_rows_alone(gpu, with_moments):
    """P = 257, n_new = 3 on the mixed case: the rows that tests/mcmc_ref.py calls neither dead nor drawn are carried over bit for
    bit in parameters, moments and statistics; the restatement says so of itself first."""
    from r2_gaussian_amd import mcmc as MC
    from r2_gaussian_amd.gaussians import activate
    P, n_new = 257, 3
    c = R.relocation_case(P, "mixed")
    p, moments, stats = _rows(gpu, c["raw"], P, with_moments)
    stats = stats if with_moments else None
    act = activate(p["density"], p["scaling"], p["rotation"], None)
    rho = act[0].cpu().numpy()
    pl = R.plan(c["raw"], rho, None, c["dead_density"], n_new, seed=2, call=P)
    em = R.emit(pl, rho, n_new)
    other = ~pl["dead"] & (pl["draws"] == 0)
    assert pl["D"] > 0 and (pl["draws"] > 0).sum() > 0 and other.sum() > 100
    assert (em["src"][:P][other] == np.arange(P)[other]).all() and not em["fresh"][:P][other].any()
    new_p, new_m, new_s, info = MC.relocate(p, moments, stats, c["dead_density"], n_new=n_new, seed=2, call=P, activated=act)
    assert info["P"] == P + n_new == new_p["xyz"].shape[0]
    assert np.array_equal(info["draws"].cpu().numpy(), pl["draws"]) and np.array_equal(info["sources"].cpu().numpy(), pl["sources"])
    _check_same((with_moments,), p, moments, stats, new_p, new_m, new_s, rows=torch.from_numpy(np.flatnonzero(other)).to(gpu))
