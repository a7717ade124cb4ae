"""CPU: the references of tests/merge_ref.py (the round-limited matching ends in the greedy one; the merged Gaussian keeps
mass, mean and second moment) and the new C ABI: header, ctypes binding and trainer flags."""
import os
import re

import numpy as np
import pytest

from tests import graph_ref as GR
from tests import merge_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("P,K", [(300, 4), (1000, 8), (2000, 16)])
def test_round_match_ends_in_the_greedy_matching(P, K):
    rng = np.random.RandomState(P + K)
    idx, d2 = GR.knn_graph(rng.uniform(-1, 1, (P, 3)).astype(np.float32), K)
    mate, rounds = R.round_match(idx, d2, np.inf)
    assert np.array_equal(mate, R.greedy_match(idx, d2, np.inf)) and 1 <= rounds <= 16
    assert R.open_count(idx, d2, np.inf, mate) == 0
    # tied, asymmetric integer costs: the two directions of a pair disagree, the pair indices break the ties
    q = rng.randint(0, 3, size=idx.shape).astype(np.float32)
    for max_cost in (0.0, 1.0, np.inf):
        mate, _ = R.round_match(idx, q, max_cost)
        assert np.array_equal(mate, R.greedy_match(idx, q, max_cost))
        assert np.array_equal(mate[mate[mate >= 0]], np.flatnonzero(mate >= 0))   # an involution


def test_path_graph_matches_one_pair_per_round():
    idx, cost = R.path_graph(40)
    mate, rounds = R.round_match(idx, cost, np.inf)
    assert rounds == 20 and np.array_equal(mate, R.greedy_match(idx, cost, np.inf)) and (mate >= 0).all()
    m3, _ = R.round_match(idx, cost, np.inf, rounds=3)
    assert (m3 >= 0).sum() == 6 and R.open_count(idx, cost, np.inf, m3) > 0
    # nothing is eligible below every cost; NaN and +inf costs are never / only with max_cost = +inf eligible
    assert (R.round_match(idx, cost, 0.5)[0] == -1).all() and (R.greedy_match(idx, cost, 0.5) == -1).all()
    bad = cost.copy()
    bad[0, 0] = np.nan
    assert R.greedy_match(idx, bad, np.inf)[0] == 1      # the other direction of the pair still carries a cost
    bad[1, 1] = np.nan
    assert R.greedy_match(idx, bad, np.inf)[0] == -1


def test_merged_gaussian_keeps_mass_mean_and_second_moment():
    xyz, density, scaling, rotation = R.random_cloud(400, 3)
    xyz[10] = xyz[11]                                              # coincident centres
    scaling[20:24], rotation[20:24] = scaling[20], rotation[20]    # equal covariances
    scaling[30:32] = 0.03                                          # triple eigenvalues
    mate = np.full(400, -1, dtype=np.int32)
    mate[0::2], mate[1::2] = np.arange(1, 400, 2), np.arange(0, 400, 2)
    out = R.merge_cloud(mate, xyz, density, scaling, rotation)
    assert out["src"].shape == (200, 2) and np.array_equal(out["src"][:, 0], np.arange(0, 400, 2))
    m, cov, x = R.mass(density, scaling), R.covariance(scaling, rotation), xyz.astype(np.float64)
    a, b = out["src"][:, 0], out["src"][:, 1]
    M = m[a] + m[b]
    mean = (m[a, None] * x[a] + m[b, None] * x[b]) / M[:, None]
    second = (m[a, None, None] * (cov[a] + x[a, :, None] * x[a, None, :]) + m[b, None, None] * (cov[b] + x[b, :, None] * x[b, None, :]))
    got_second = M[:, None, None] * (out["cov"] + out["xyz"][:, :, None] * out["xyz"][:, None, :])
    assert np.allclose(out["mass"], M, rtol=1e-14, atol=0)
    assert np.allclose(out["xyz"], mean, rtol=1e-13, atol=1e-15)
    assert np.allclose(got_second, second, rtol=1e-12, atol=1e-18)
    # the stored parameterisation rebuilds the covariance and the mass; scales descend; the quaternion is canonical
    rebuilt = R.covariance(out["scaling"], out["rotation"])
    err = np.linalg.norm(rebuilt - out["cov"], axis=(1, 2)) / np.linalg.norm(out["cov"], axis=(1, 2))
    assert err.max() < 1e-12, err.max()
    assert np.allclose(R.mass(out["density"], out["scaling"]), M, rtol=1e-13, atol=0)
    s, q = out["scaling"], out["rotation"]
    assert (s[:, 0] >= s[:, 1]).all() and (s[:, 1] >= s[:, 2]).all() and (s[:, 2] > 0).all()
    assert np.allclose(np.linalg.norm(q, axis=1), 1, rtol=0, atol=1e-14) and (q[:, 0] >= 0).all()
    assert (np.linalg.det(R.quat_to_rot(q)) > 0).all()


def test_cost_reference_properties():
    xyz, density, scaling, rotation = R.random_cloud(200, 5)
    idx, _ = GR.knn_graph(xyz, 4)
    c = R.edge_costs(idx, xyz, density, scaling, rotation)
    assert np.isfinite(c).all() and (c >= 0).all()
    # invariant under a common scaling of the cloud; 0 for two copies of one Gaussian
    c2 = R.edge_costs(idx, 8 * xyz.astype(np.float64), density, 8 * scaling.astype(np.float64), rotation)
    assert np.allclose(c, c2, rtol=1e-9, atol=1e-12)
    two = [np.repeat(t[:1], 2, 0) for t in (xyz, density, scaling, rotation)]
    assert R.edge_costs(np.array([[1], [0]]), *two).max() < 1e-12
    # +inf: invalid and self edges, a density <= 0, a NaN scale, a trace beyond the bound
    idx2 = idx.copy()
    idx2[0, 0], idx2[1, 0] = -1, 1
    density2, scaling2 = density.copy(), scaling.copy()
    density2[5], scaling2[6, 1] = 0.0, np.nan
    c = R.edge_costs(idx2, xyz, density2, scaling2, rotation)
    assert np.isposinf(c[0, 0]) and np.isposinf(c[1, 0]) and np.isposinf(c[5]).all() and np.isposinf(c[6]).all()
    assert np.isposinf(c[idx2 == 5]).all() and np.isposinf(c[idx2 == 6]).all()
    assert np.isposinf(R.edge_costs(idx, xyz, density, scaling, rotation, max_trace=1e-12)).all()


NEW_SYMBOLS = ("r2_merge_cost", "r2_graph_match_workspace_bytes", "r2_graph_match", "r2_merge_scratch_bytes", "r2_merge_count",
               "r2_merge_emit")


def test_header_binding_and_module_agree():
    from r2_gaussian_amd import _lib
    from r2_gaussian_amd import merge as MG
    src = open(os.path.join(ROOT, "include", "r2hip.h")).read()
    for s in NEW_SYMBOLS:
        assert re.search(r"R2_API\s+(int|size_t)\s+%s\s*\(" % s, src), s
        assert s in _lib.exported_symbols()
    for name in ("R2_MERGE_HUB", "R2_MERGE_JACOBI_SWEEPS"):
        m = re.search(r"^#define\s+%s\s+(-?\d+)\s*$" % name, src, flags=re.M)
        assert m and int(m.group(1)) == getattr(_lib, name), name
    assert re.search(r"^#define\s+R2_ABI_VERSION\s+3\s*$", src, flags=re.M) and _lib.R2_ABI_VERSION == 3
    L = _lib.lib()   # argtypes on every symbol; raises on a missing one
    assert L.r2_abi_version() == 3
    assert L.r2_graph_match_workspace_bytes(0) == 0 and L.r2_graph_match_workspace_bytes(65) == 512
    assert L.r2_merge_scratch_bytes(0) == 0 and L.r2_merge_scratch_bytes(1000) >= 5 * 4096
    for name in ("merge_costs", "match_edges", "merge_pairs", "merge_gaussians"):
        assert hasattr(MG, name)
    # the trace bound never exceeds max_scale^2
    for hi in (0.1, 0.3, 1.0 / 3.0, 2.5):
        t = MG.max_trace_of(hi)
        assert np.float32(t) == t and t <= hi * hi < float(np.nextafter(np.float32(t), np.float32(np.inf)))
    assert MG.max_trace_of(None) == 0.0
    with pytest.raises(ValueError):
        MG.max_trace_of(-1.0)


def test_trainer_flags_default_off():
    from r2_gaussian_amd import train as TR
    from r2_gaussian_amd.gaussians import GaussianModel
    a = TR.build_parser().parse_args(["-s", "x"])
    assert a.merge_interval == 0 and a.merge_cost == 0.1 and a.merge_k == 8
    assert a.merge_from_iter == 500 and a.merge_until_iter == 15000
    a = TR.build_parser().parse_args(["-s", "x", "--merge_interval", "200", "--merge_cost", "0.05", "--merge_k", "4",
                                      "--merge_from_iter", "10", "--merge_until_iter", "90"])
    assert (a.merge_interval, a.merge_cost, a.merge_k, a.merge_from_iter, a.merge_until_iter) == (200, 0.05, 4, 10, 90)
    assert callable(GaussianModel.merge)
