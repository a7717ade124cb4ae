"""CPU: the restatement of the Fisher / variance entries (tests/gaussian_fisher_ref.py) against autograd's Jacobian, the identity
between the Fisher diagonal and the projection variance, the measured float32 error the GPU tolerance is taken from and the
condition that keeps that tolerance meaningful, the noise model of ``noise_weights``, and the host-side pieces of
r2_gaussian_amd.uncertainty."""
import os
import re

import numpy as np
import pytest
import torch

from tests import gaussian_field_ref as RF
from tests import gaussian_fisher_ref as R
from tests import gaussian_project_ref as RP

ENTRIES = ("r2_project_gaussians_fisher", "r2_query_gaussians_variance", "r2_project_gaussians_variance")


def _jacobians(f, cloud):
    """d f / d (xyz, density, scaling, rotation) of a float64 torch function of the four parameter tensors: -> [11, P] lists
    of rows, each [outputs]: J[t][i] = d f / d parameter t of Gaussian i."""
    leaves = tuple(torch.from_numpy(np.asarray(a, np.float64)) for a in cloud)
    J = torch.autograd.functional.jacobian(f, leaves)
    P = leaves[0].shape[0]
    rows = []
    for j, cols in zip(J, (3, 1, 3, 4)):
        j = j.reshape(-1, P, cols)
        rows += [j[:, :, c] for c in range(cols)]
    return torch.stack(rows).numpy()   # [11, outputs, P]


@pytest.mark.parametrize("name", ["cone_p1", "parallel_p1", "cone_p7"])
def test_fisher64_is_the_weighted_sum_of_squared_jacobian_entries(name):
    """The float64 restatement of r2_project_gaussians_fisher (every pair) = sum_pixels w J^2 with J from
    torch.autograd.functional.jacobian of gaussian_project_ref.torch_image, to 1e-10 of F; and the projection variance =
    sum_it v J^2 per pixel."""
    r = R.projector_reference(name)
    sc = r["scene"]
    f = lambda x, d, s, q: RP.torch_image(sc["rays"], sc["cone"], sc["H"], sc["W"], x, d, s, q, sc["mod"]).reshape(-1)
    J = _jacobians(f, sc["cloud"])
    w = r["weights"].astype(np.float64).reshape(1, -1, 1)
    want = (w * J * J).sum(1)
    assert want.max() > 0
    assert (np.abs(r["F"][1] - want) <= 1e-10 * want).all()
    v = R.stack(r["var"], np.float64)[:, None, :]
    pv = (v * J * J).sum((0, 2))
    assert (np.abs(r["pv"][1].reshape(-1) - pv) <= 1e-10 * pv).all()


@pytest.mark.parametrize("name", ["tail_1", "raw_quat"])
def test_field_variance64_is_the_sum_of_squared_jacobian_entries(name):
    """The same for r2_query_gaussians_variance, against the Jacobian of gaussian_field_ref.torch_field."""
    r = R.field_reference(name)
    sc = r["scene"]
    pts = torch.from_numpy(sc["points"].reshape(-1, 3).astype(np.float64))
    J = _jacobians(lambda x, d, s, q: RF.torch_field(pts, x, d, s, q, sc["mod"]), sc["cloud"])
    v = R.stack(r["var"], np.float64)[:, None, :]
    want = (v * J * J).sum((0, 2))
    assert want.max() > 0
    assert (np.abs(r["pv"][1] - want) <= 1e-10 * want).all()


@pytest.mark.parametrize("name", R.IDENTITY_SCENES)
def test_identity_between_fisher_and_projection_variance(name):
    """sum_pixels w * projection_variance = sum_it F_it v_it: the same pairs added in two orders; float64, 1e-12, both limits."""
    r = R.projector_reference(name)
    w = r["weights"].astype(np.float64)
    for b in range(2):
        total = float((w * r["pv"][b]).sum())
        assert total > 0 and abs(total - r["T"][b]) <= 1e-12 * total


def test_bracket_is_monotone():
    """Sums of squares: the float64 sum over the pairs with q <= 32 is nowhere above the sum over every pair."""
    for name in ("cone_p300", "parallel_small_sigma"):
        r = R.projector_reference(name)
        assert (r["F"][0] <= r["F"][1]).all() and (r["pv"][0] <= r["pv"][1]).all()
    r = R.field_reference("plane")
    assert (r["pv"][0] <= r["pv"][1]).all() and (r["pv"][0] < r["pv"][1]).any()


def test_stored_e32_matches_a_fresh_measurement_and_stays_below_a_tenth():
    """tests/golden/gaussian_fisher/e32.json (python -m tests.gaussian_fisher_ref) within 10 % of a fresh measurement, and
    every e32 below 0.1: 4 x e32 then stays well under 1, so a kernel that is wrong by a factor cannot pass."""
    stored, fresh = R.load_e32(), R.measure_e32()
    assert sorted(stored["fisher"]) == sorted(R.PROJ_SCENES) == sorted(stored["projection_variance"])
    assert sorted(stored["field_variance"]) == sorted(R.FIELD_SCENES)
    flat = lambda d: {(q, n, g): v for q in d for n in d[q] for g, v in (d[q][n].items() if isinstance(d[q][n], dict) else [("", d[q][n])])}
    a, b = flat(stored), flat(fresh)
    assert sorted(a) == sorted(b)
    for k in a:
        assert abs(a[k] - b[k]) <= 0.1 * b[k], (k, a[k], b[k])
        assert a[k] < 0.1, (k, a[k])


def test_rotated_candidate_is_more_informative_in_float64():
    """The end-to-end case of the GPU test, in the float64 restatement: the candidate that is a training view scores at least
    10 % lower than that view rotated by 90 degrees."""
    from r2_gaussian_amd import projector
    E = R.END_TO_END
    sc = R.proj_scene(E["scene"])
    rays = projector.ray_params(R.candidate_views(), (1.0, 1.0, 1.0), (0.0, 0.0, 0.0), (1, 1, 1))
    assert np.array_equal(rays[E["seen"]], sc["rays"][0])
    s = R.information64()
    print("view information, float64:", s)
    assert (s > 0).all() and s[E["seen"]] <= s[E["unseen"]] / 1.1


def test_noise_weights_match_the_sample_variance_of_add_noise():
    """1 / noise_weights against the sample variance of datagen.add_noise over 4000 draws of one small stack, pixel by pixel,
    within three standard errors of that sample variance, SE^2 = (m4 - s^4 (n - 3) / (n - 1)) / n from the sample's own
    fourth central moment m4.  The stack stays well above 0 (the clip of negatives never acts) and the counts well above the
    additive noise (the first-order expansion of the logarithm is off by about 1 / Ibar, 3e-5 of the variance)."""
    from r2_gaussian_amd import datagen as D
    from r2_gaussian_amd.uncertainty import noise_weights
    projs = (0.5 + 1.5 * np.random.RandomState(3).rand(2, 3, 4)).astype(np.float32)
    i0, gaussian, n = 1e5, (0.0, 10.0), 4000
    rng = np.random.RandomState(4)
    draws = np.stack([D.add_noise(projs, i0, gaussian, rng).astype(np.float64) for _ in range(n)])
    assert (draws > 0).all()
    mean = draws.mean(0)
    c = draws - mean
    s2 = (c ** 2).sum(0) / (n - 1)
    m4 = (c ** 4).mean(0)
    se = np.sqrt((m4 - s2 ** 2 * (n - 3) / (n - 1)) / n)
    w = noise_weights(projs, i0, gaussian)
    assert isinstance(w, np.ndarray) and w.dtype == np.float32 and w.shape == projs.shape
    dev = np.abs(1.0 / w.astype(np.float64) - s2) / se
    print("noise_weights: worst |1 / w - s^2| in standard errors %.2f; relative standard error %.3f" % (dev.max(), (se / s2).max()))
    assert (dev <= 3.0).all()
    # the maximum may be given; a tensor gives a tensor; an all-zero stack, which add_noise leaves alone, gives ones
    assert np.array_equal(noise_weights(projs, i0, gaussian, m=float(projs.max())), w)
    wt = noise_weights(torch.from_numpy(projs), i0, gaussian)
    assert isinstance(wt, torch.Tensor) and wt.dtype == torch.float32 and np.array_equal(wt.numpy(), w)
    assert np.array_equal(noise_weights(np.zeros((2, 3, 4), np.float32), i0, gaussian), np.ones((2, 3, 4), np.float32))


def test_parameter_variance_and_its_argument_checks():
    from r2_gaussian_amd.uncertainty import CloudTuple, parameter_variance
    F = CloudTuple(torch.tensor([[0.0, 1.0, 3.0]]), torch.tensor([[7.0]]), torch.zeros((1, 3)), torch.ones((1, 4)))
    v = parameter_variance(F, 1.0)
    assert isinstance(v, CloudTuple) and torch.equal(v.xyz, torch.tensor([[1.0, 0.5, 0.25]])) and torch.equal(v.density, torch.tensor([[0.125]]))
    v = parameter_variance(tuple(F), (1.0, 1.0, 4.0, 3.0))
    assert torch.equal(v.scaling, torch.full((1, 3), 0.25)) and torch.equal(v.rotation, torch.full((1, 4), 0.25))
    for bad in (0.0, -1.0, float("nan"), float("inf"), (1.0, 1.0, 0.0, 1.0), (1.0, 1.0, 1.0)):
        with pytest.raises(ValueError):
            parameter_variance(F, bad)
    with pytest.raises(ValueError):
        parameter_variance(F[:3], 1.0)
    with pytest.raises(ValueError):
        parameter_variance((F.xyz, F.density, F.scaling, None), 1.0)


def test_header_declares_and_the_binding_binds_the_three_entries():
    from r2_gaussian_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "r2hip.h")) as f:
        header = f.read()
    assert "#define R2_ABI_VERSION 3" in header and _lib.R2_ABI_VERSION == 3   # the entries are additive
    for name in ENTRIES:
        assert re.search(r"R2_API int %s\(" % name, header), name
        assert name in _lib.exported_symbols()
    res, args = _lib._SIGNATURES["r2_project_gaussians_fisher"]
    assert len(args) == 17 and len(_lib._SIGNATURES["r2_query_gaussians_variance"][1]) == 14
    assert len(_lib._SIGNATURES["r2_project_gaussians_variance"][1]) == 17


def test_train_flag_is_off_by_default():
    from r2_gaussian_amd import train as TR
    ap = TR.build_parser()
    assert ap.parse_args(["-s", "x"]).save_uncertainty is None
    assert ap.parse_args(["-s", "x", "--save_uncertainty", "0.5"]).save_uncertainty == 0.5
