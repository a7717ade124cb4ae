"""GPU: merging of neighbouring Gaussians (r2_gaussian_amd.merge; include/r2hip.h: r2_merge_cost, r2_graph_match,
r2_merge_count, r2_merge_emit) against the float64 references of tests/merge_ref.py.

Bounds (tests/merge_ref.py): a cost is a double rounded once, |got - ref| <= 2^-23 |ref| + 1e-9; the matching is exact
(array_equal with the round-limited rule and, once nothing is open, with the sequential greedy matching); a merged row, read
back in float64 from its float outputs, keeps the mean within 2^-23, the covariance within 2^-20 of its Frobenius norm (16
roundings) and the mass within 2^-21 (8 roundings).  Every check prints the largest fraction of its bound that it used."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import merge_ref as R

pytestmark = pytest.mark.gpu
SIZES = (0, 1, 2, 63, 64, 65, 257, 1000)
KS = (1, 4, 16)


@functools.lru_cache(maxsize=None)
def _cloud(P):
    return R.random_cloud(P, 100 + P)


def _dev(arrays, gpu):
    return [torch.as_tensor(a).to(gpu) for a in arrays]


@functools.lru_cache(maxsize=None)
def _knn_case(P, K):
    """(graph, device parameters, cost of the kernel as numpy, float64 reference cost): computed once, never modified."""
    from r2_gaussian_amd import graph as G
    from r2_gaussian_amd import merge as MG
    gpu = torch.device("cuda:0")
    cloud = _cloud(P)
    dev = _dev(cloud, gpu)
    g = G.knn_graph(dev[0], K)
    cost = MG.merge_costs(g, *dev)
    idx = g.idx.cpu().numpy()
    return g, dev, cost, idx, R.edge_costs(idx, *cloud)


def _graph(idx, gpu):
    from r2_gaussian_amd import graph as G
    return G.graph_from_indices(torch.as_tensor(np.asarray(idx, dtype=np.int32)).to(gpu))


def _match(g, cost, max_cost, rounds):
    from r2_gaussian_amd import merge as MG
    c = cost if torch.is_tensor(cost) else torch.as_tensor(np.asarray(cost, dtype=np.float32)).to(g.idx.device)
    return MG.match_edges(g, c, max_cost, rounds=rounds).cpu().numpy()


# ------------------------------------------------------------------------------------------------ cost
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("P", SIZES)
def test_cost_against_float64(gpu, P, K):
    g, _dev_p, cost, idx, ref = _knn_case(P, K)
    got = cost.cpu().numpy()
    assert got.shape == (P, K) and got.dtype == np.float32
    fin = np.isfinite(ref)
    assert np.array_equal(np.isposinf(got), ~fin) and np.array_equal(fin, idx >= 0)
    if fin.any():
        err = np.abs(got[fin].astype(np.float64) - ref[fin])
        bound = R.COST_REL * np.abs(ref[fin]) + R.COST_ABS
        print("cost P %d K %d: %d edges, largest fraction of the bound %.3g, cost range %.3g .. %.3g"
              % (P, K, fin.sum(), (err / bound).max(), ref[fin].min(), ref[fin].max()))
        assert (err <= bound).all()
        assert (got[fin] >= 0).all()
    # cost[i -> j] and cost[j -> i] carry the same bits wherever both edges exist
    both = 0
    bits = got.view(np.uint32)
    for i in range(P):
        for k in range(K):
            j = idx[i, k]
            if j >= 0:
                back = np.flatnonzero(idx[j] == i)
                if back.size:
                    both += 1
                    assert bits[i, k] == bits[j, back[0]], (i, j)
    assert both > 0 or P < 2


def test_cost_is_inf_where_the_contract_says(gpu):
    from r2_gaussian_amd import merge as MG
    P, K = 65, 4
    xyz, density, scaling, rotation = (a.copy() for a in _cloud(P))
    rng = np.random.RandomState(7)
    idx = rng.randint(0, P, size=(P, K)).astype(np.int32)
    idx[0, 0], idx[1, 1], idx[2, 2], idx[3, 3] = -1, P, 2, 3          # missing, out of range, a self edge (row 2), row 3 -> 3
    density[5], density[6] = 0.0, -1.0
    scaling[7, 1], scaling[8, 0], rotation[9, 2], xyz[10, 0] = np.nan, 0.0, np.inf, np.nan
    g = _graph(idx, gpu)
    dev = _dev((xyz, density, scaling, rotation), gpu)
    got = MG.merge_costs(g, *dev).cpu().numpy()
    ref = R.edge_costs(idx, xyz, density, scaling, rotation)
    assert np.array_equal(np.isposinf(got), np.isposinf(ref)) and not np.isnan(got).any()
    fin = np.isfinite(ref)
    assert fin.sum() > 100 and (np.abs(got[fin] - ref[fin]) <= R.COST_REL * np.abs(ref[fin]) + R.COST_ABS).all()
    assert np.isposinf(got[0, 0]) and np.isposinf(got[1, 1]) and np.isposinf(got[2, 2]) and np.isposinf(got[3, 3])
    for bad in (5, 6, 7, 8, 9, 10):
        assert np.isposinf(got[bad]).all() and np.isposinf(got[idx == bad]).all(), bad
    # beyond max_trace: exactly the edges whose merged trace exceeds the float bound
    hi = 0.6
    got = MG.merge_costs(g, *dev, max_scale=hi).cpu().numpy()
    ref_t = R.edge_costs(idx, xyz, density, scaling, rotation, max_trace=MG.max_trace_of(hi))
    assert np.array_equal(np.isposinf(got), np.isposinf(ref_t))
    assert np.isposinf(ref_t).sum() > np.isposinf(ref).sum() and np.isfinite(ref_t).sum() > 0


def test_argument_errors(gpu):
    from r2_gaussian_amd import _lib
    from r2_gaussian_amd import merge as MG
    L = _lib.lib()
    t = torch.zeros(64, dtype=torch.float32, device=gpu)
    p = t.data_ptr()
    assert L.r2_merge_cost(0, 4, None, None, None, None, None, 0.0, None, None) == 0
    assert L.r2_graph_match(0, 4, None, None, None, None, 1.0, 3, None, None, 0, None) == 0
    counts = (C.c_uint * 2)(7, 7)
    assert L.r2_merge_count(0, 4, None, None, None, None, 1.0, None, None, None, None, counts, None) == 0 and list(counts) == [0, 0]
    assert L.r2_merge_emit(0, None, None, None, None, None, 0, None, None, None, None, None, None) == 0
    for P, K in ((4, 0), (-1, 4), (1 << 20, 1 << 11)):
        assert L.r2_merge_cost(P, K, p, p, p, p, p, 0.0, p, None) == _lib.R2_ERR_INVALID
        assert L.r2_graph_match(P, K, p, p, p, p, 1.0, 3, p, p, 1 << 30, None) == _lib.R2_ERR_INVALID
        assert L.r2_merge_count(P, K, p, p, p, p, 1.0, p, p, p, p, counts, None) == _lib.R2_ERR_INVALID
    assert L.r2_merge_cost(4, 2, None, p, p, p, p, 0.0, p, None) == _lib.R2_ERR_INVALID
    assert L.r2_graph_match(4, 2, p, p, p, p, 1.0, 3, p, None, 0, None) == _lib.R2_ERR_INVALID      # no workspace
    assert L.r2_graph_match(4, 2, p, p, p, p, 1.0, -1, p, p, 256, None) == _lib.R2_ERR_INVALID      # rounds < 0
    assert L.r2_merge_emit(4, p, p, p, p, p, 5, p, p, p, p, p, None) == _lib.R2_ERR_INVALID         # more rows out than in
    g, dev, cost, _idx, _ref = _knn_case(64, 4)
    with pytest.raises(ValueError):
        MG.merge_costs(g, dev[0][:10], *dev[1:])
    with pytest.raises(ValueError):
        MG.match_edges(g, cost[:, :2], 1.0)
    with pytest.raises(ValueError):
        MG.merge_pairs(g, cost, 1.0, torch.zeros(3, dtype=torch.int32, device=gpu), *dev)
    with pytest.raises(ValueError):
        MG.merge_costs("graph", *dev)
    with pytest.raises(_lib.R2HipError):
        MG.merge_costs(g, dev[0].cpu(), *dev[1:])


# ------------------------------------------------------------------------------------------------ match
def _check_match(g, idx, cost_np, max_cost, label):
    """rounds 1, 2, 3 against the round-limited rule; then enough rounds for nothing to be open: the greedy matching."""
    from r2_gaussian_amd import merge as MG
    cost_t = torch.as_tensor(cost_np).to(g.idx.device)
    for rounds in (1, 2, 3):
        want, _ = R.round_match(idx, cost_np, max_cost, rounds=rounds)
        assert np.array_equal(_match(g, cost_t, max_cost, rounds), want), (label, rounds)
    full, needed = R.round_match(idx, cost_np, max_cost)
    got = _match(g, cost_t, max_cost, needed)
    greedy = R.greedy_match(idx, cost_np, max_cost)
    assert np.array_equal(full, greedy)
    assert np.array_equal(got, greedy), label
    assert np.array_equal(_match(g, cost_t, max_cost, needed + 5), greedy)          # further rounds change nothing
    # open, as the count kernel reports it (any parameters with positive mass do)
    P = idx.shape[0]
    ones = [torch.ones((P, w), dtype=torch.float32, device=g.idx.device) for w in (3, 1, 3, 4)]
    for rounds in (1, needed):
        mate = MG.match_edges(g, cost_t, max_cost, rounds=rounds)
        info = MG.merge_pairs(g, cost_t, max_cost, mate, *ones)[5]
        m = mate.cpu().numpy()
        assert info["open"] == R.open_count(idx, cost_np, max_cost, m), (label, rounds)
        assert info["pairs"] == (m >= 0).sum() // 2 and info["P"] == P - info["pairs"]
    assert info["open"] == 0
    print("%s: P %d, %d pairs, %d rounds to a maximal matching" % (label, P, (greedy >= 0).sum() // 2, needed))
    return needed


@pytest.mark.parametrize("P,K", [(2, 1), (63, 4), (64, 16), (65, 1), (257, 4), (1000, 4), (1000, 16)])
def test_match_on_knn_graphs(gpu, P, K):
    g, _dev_p, cost, idx, _ref = _knn_case(P, K)
    cost_np = cost.cpu().numpy()
    finite = cost_np[np.isfinite(cost_np)]
    needed = _check_match(g, idx, cost_np, np.inf, "knn costs, max_cost inf")
    assert needed <= 16
    _check_match(g, idx, cost_np, float(np.median(finite)), "knn costs, max_cost = median")
    # three cost values, the two directions of a pair drawn independently: ties everywhere, broken by the pair's indices
    q = np.random.RandomState(P * 31 + K).randint(0, 3, size=idx.shape).astype(np.float32)
    _check_match(g, idx, q, 1.0, "quantised costs")
    # below every cost nothing matches
    assert (_match(g, cost, float(finite.min()) * 0.5 - 1e-30, 4) == -1).all()
    # two calls give the same bits
    assert np.array_equal(_match(g, cost, np.inf, 2), _match(g, cost, np.inf, 2))


def test_match_path_takes_one_pair_per_round(gpu):
    idx, cost = R.path_graph(40)
    g = _graph(idx, gpu)
    m3 = _match(g, cost, np.inf, 3)
    assert (m3 >= 0).sum() == 6 and np.array_equal(m3, R.round_match(idx, cost, np.inf, rounds=3)[0])
    assert _check_match(g, idx, cost, np.inf, "path of 40") == 20


def test_match_hubs_are_walked_by_the_wave(gpu):
    # a star: 1000 spokes point at node 0, which has no edges of its own: its partner comes from its incoming list alone
    n = 1000
    rng = np.random.RandomState(3)
    idx = np.zeros((n + 1, 1), dtype=np.int32)
    idx[0, 0] = -1
    cost = rng.uniform(1, 2, size=(n + 1, 1)).astype(np.float32)
    g = _graph(idx, gpu)
    assert int(g.in_offsets[1]) == n
    mate = _match(g, cost, np.inf, 1)
    best = 1 + int(np.argmin(cost[1:, 0]))
    assert mate[0] == best and mate[best] == 0 and (mate >= 0).sum() == 2
    assert _check_match(g, idx, cost, np.inf, "star") == 1
    # ties: every spoke costs the same, the lowest index wins
    assert _match(g, np.ones_like(cost), np.inf, 1)[0] == 1
    # two hubs in one wave (nodes 0 and 1), every other node points at both, and a few hubs further on (nodes 70, 300)
    idx2 = np.zeros((n + 2, 3), dtype=np.int32)
    idx2[:, 1] = 1
    idx2[:, 2] = np.where(np.arange(n + 2) % 2 == 0, 70, 300)
    idx2[0], idx2[1] = (-1, 1, -1), (0, -1, -1)
    cost2 = rng.randint(0, 50, size=idx2.shape).astype(np.float32)
    _check_match(_graph(idx2, gpu), idx2, cost2, np.inf, "four hubs")
    _check_match(_graph(idx2, gpu), idx2, cost2, 10.0, "four hubs, max_cost 10")


def test_match_ignores_nan_and_takes_inf_only_at_inf(gpu):
    g, _dev_p, cost, idx, _ref = _knn_case(257, 4)
    c = cost.cpu().numpy().copy()
    rng = np.random.RandomState(11)
    c[rng.rand(*c.shape) < 0.2] = np.nan
    c[rng.rand(*c.shape) < 0.2] = np.inf
    c[rng.rand(*c.shape) < 0.05] = -np.inf
    _check_match(g, idx, c, np.inf, "nan / inf costs, max_cost inf")
    _check_match(g, idx, c, 1e30, "nan / inf costs, max_cost 1e30")
    assert (_match(g, np.full_like(c, np.nan), np.inf, 3) == -1).all()


# ------------------------------------------------------------------------------------------------ count / emit
def _emit_guarded(g, cost, max_cost, mate, dev, guard=3):
    """r2_merge_count + r2_merge_emit through the C ABI with NaN / sentinel guard rows around every output."""
    from r2_gaussian_amd import _lib
    L = _lib.lib()
    P, K = g.P, g.K
    gpu = g.idx.device
    scratch = torch.empty(int(L.r2_merge_scratch_bytes(P)), dtype=torch.uint8, device=gpu)
    counts = (C.c_uint * 2)()
    s = torch.cuda.current_stream(gpu).cuda_stream
    rc = L.r2_merge_count(P, K, g.idx.data_ptr(), g.in_offsets.data_ptr(), g.in_edges.data_ptr(), cost.data_ptr(), float(max_cost),
                          mate.data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), scratch.data_ptr(), counts, s)
    assert rc == 0
    Pn = P - int(counts[0])
    outs = [torch.full((Pn + 2 * guard, w), float("nan"), dtype=torch.float32, device=gpu) for w in (3, 1, 3, 4)]
    src = torch.full((Pn + 2 * guard, 2), -77, dtype=torch.int32, device=gpu)
    rc = L.r2_merge_emit(P, dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), dev[3].data_ptr(), scratch.data_ptr(), Pn,
                         *[o[guard:].data_ptr() for o in outs], src[guard:].data_ptr(), s)
    assert rc == 0
    torch.cuda.synchronize(gpu)
    for o in outs:
        assert bool(torch.isnan(o[:guard]).all()) and bool(torch.isnan(o[Pn + guard:]).all())
    assert bool((src[:guard] == -77).all()) and bool((src[Pn + guard:] == -77).all())
    return [o[guard:Pn + guard].cpu().numpy() for o in outs], src[guard:Pn + guard].cpu().numpy(), (int(counts[0]), int(counts[1]))


def _check_rows(outs, src, mate, cloud, label):
    """The emitted rows against the float64 reference of the same mate array -> (cov, mass) maxima in float roundings."""
    ref = R.merge_cloud(mate, *cloud)
    assert np.array_equal(src, ref["src"]), label
    xyz, density, scaling, rotation = outs
    single = src[:, 1] < 0
    for got, inp in zip(outs, cloud):            # unmerged rows: bit copies
        a = np.ascontiguousarray(got[single]).view(np.uint32)
        b = np.ascontiguousarray(np.asarray(inp).reshape(len(inp), -1)[src[single, 0]]).view(np.uint32)
        assert np.array_equal(a, b), label
    m = ~single
    if not m.any():
        return 0.0, 0.0
    x64 = np.asarray(cloud[0], dtype=np.float64)
    big = np.maximum(np.abs(x64[src[m, 0]]), np.abs(x64[src[m, 1]]))
    mu_err = np.abs(xyz[m].astype(np.float64) - ref["xyz"][m])
    assert (mu_err <= R.MU_REL * np.abs(ref["xyz"][m]) + R.MU_REL * big).all(), label
    rebuilt = R.covariance(scaling[m].astype(np.float64), rotation[m].astype(np.float64))
    cov_err = np.linalg.norm(rebuilt - ref["cov"][m], axis=(1, 2)) / np.linalg.norm(ref["cov"][m], axis=(1, 2))
    mass_err = np.abs(R.mass(density[m], scaling[m]) - ref["mass"][m]) / ref["mass"][m]
    print("%s: %d merged rows, covariance %.2f roundings (bound 16), mass %.2f roundings (bound 8), mean %.2f of its bound"
          % (label, m.sum(), cov_err.max() / R.U, mass_err.max() / R.U,
             (mu_err / (R.MU_REL * np.abs(ref["xyz"][m]) + R.MU_REL * big + 1e-300)).max()))
    assert (cov_err <= R.COV_REL).all() and (mass_err <= R.MASS_REL).all(), label
    s, q = scaling[m].astype(np.float64), rotation[m].astype(np.float64)
    assert (s[:, 0] >= s[:, 1]).all() and (s[:, 1] >= s[:, 2]).all() and (s[:, 2] > 0).all(), label
    assert (np.abs(np.linalg.norm(q, axis=1) - 1) <= 2.0 ** -22).all() and (q[:, 0] >= 0).all(), label
    return cov_err.max() / R.U, mass_err.max() / R.U


@pytest.mark.parametrize("P,K", [(2, 1), (63, 4), (65, 16), (257, 4), (1000, 4), (1000, 16)])
def test_emit_after_a_matching(gpu, P, K):
    from r2_gaussian_amd import merge as MG
    g, dev, cost, idx, _ref = _knn_case(P, K)
    max_cost = float(np.median(cost.cpu().numpy()[np.isfinite(cost.cpu().numpy())]))
    mate = MG.match_edges(g, cost, max_cost, rounds=16)
    outs, src, (pairs, n_open) = _emit_guarded(g, cost, max_cost, mate, dev)
    assert pairs > 0 and n_open == 0 and len(src) == P - pairs
    _check_rows(outs, src, mate.cpu().numpy(), _cloud(P), "emit P %d K %d" % (P, K))
    # the Python entry point returns the same rows, and the same bits on a second call
    a = MG.merge_pairs(g, cost, max_cost, mate, *dev)
    b = MG.merge_pairs(g, cost, max_cost, mate, *dev)
    for t, u, o in zip(a[:4], b[:4], outs):
        assert torch.equal(t, u) and np.array_equal(t.cpu().numpy().view(np.uint32), o.view(np.uint32))
    assert np.array_equal(a[4].cpu().numpy(), src) and a[5] == dict(pairs=pairs, open=0, P=P - pairs)


def test_emit_degenerate_pairs(gpu):
    """Equal covariances, triple eigenvalues, coincident centres, 100 : 1 needles at right angles, very unequal masses."""
    P = 64
    xyz, density, scaling, rotation = (a.copy() for a in R.random_cloud(P, 9))
    xyz[1], density[1], scaling[1], rotation[1] = xyz[0], density[0], scaling[0], rotation[0]   # two copies of one Gaussian
    scaling[2:4] = 0.03; rotation[2:4] = (1, 0, 0, 0)                                     # two spheres
    xyz[5] = xyz[4]                                                                      # coincident centres
    scaling[6], scaling[7], rotation[6:8] = (1.0, 0.01, 0.01), (0.01, 1.0, 0.01), (1, 0, 0, 0)   # needles at right angles
    density[8], density[9] = 1e-6, 50.0
    scaling[10:12] = 0.02; rotation[10:12] = (1, 0, 0, 0); xyz[11] = xyz[10] + np.float32([0, 0, 0.5])   # spheres apart along z
    mate = (np.arange(P) ^ 1).astype(np.int32)
    g = _graph(mate[:, None], gpu)
    dev = _dev((xyz, density, scaling, rotation), gpu)
    cost = torch.zeros((P, 1), dtype=torch.float32, device=gpu)
    outs, src, (pairs, n_open) = _emit_guarded(g, cost, 1.0, torch.as_tensor(mate).to(gpu), dev)
    assert pairs == P // 2 and n_open == 0                                              # every node matched
    _check_rows(outs, src, mate, (xyz, density, scaling, rotation), "degenerate pairs")
    assert np.allclose(outs[2][0], np.sort(scaling[0])[::-1], rtol=1e-6) and np.allclose(outs[1][0], 2 * density[0], rtol=1e-6)


def test_bad_mates_count_as_unmatched(gpu):
    from r2_gaussian_amd import merge as MG
    P, K = 257, 4
    g, dev, cost, idx, _ref = _knn_case(P, K)
    cloud = _cloud(P)
    good = MG.match_edges(g, cost, np.inf, rounds=16).cpu().numpy()
    pairs = [(i, good[i]) for i in range(P) if good[i] > i]
    assert len(pairs) > 40
    bad = good.copy()
    (a0, b0), (a1, b1), (a2, b2), (a3, b3), (a4, b4) = pairs[:5]
    bad[a0] = P                 # out of range (its partner is then one-sided)
    bad[a1] = -5
    bad[b2] = 10 ** 6
    bad[a3] = a3                # a self mate
    bad[b4] = a0                # not an involution
    outs, src, (n_pairs, _open) = _emit_guarded(g, cost, np.inf, torch.as_tensor(bad).to(gpu), dev)
    assert n_pairs == len(pairs) - 5
    _check_rows(outs, src, bad, cloud, "bad mates")
    # a pair with an end of non-positive or non-finite mass is no pair
    density = cloud[1].copy()
    a5, b5 = pairs[5]
    a6, b6 = pairs[6]
    density[a5], density[b6] = -1.0, np.inf
    dev2 = [dev[0], torch.as_tensor(density).to(gpu), dev[2], dev[3]]
    outs, src, (n_pairs, _open) = _emit_guarded(g, cost, np.inf, torch.as_tensor(good).to(gpu), dev2)
    assert n_pairs == len(pairs) - 2
    _check_rows(outs, src, good, (cloud[0], density, cloud[2], cloud[3]), "bad masses")
    # pairs at the first and the last index only; no node matched
    only = np.full(P, -1, dtype=np.int32)
    only[0], only[P - 1] = P - 1, 0
    outs, src, (n_pairs, _open) = _emit_guarded(g, cost, np.inf, torch.as_tensor(only).to(gpu), dev)
    assert n_pairs == 1 and src[0].tolist() == [0, P - 1] and src[-1].tolist() == [P - 2, -1]
    _check_rows(outs, src, only, cloud, "first with last")
    none = np.full(P, -1, dtype=np.int32)
    outs, src, (n_pairs, n_open) = _emit_guarded(g, cost, np.inf, torch.as_tensor(none).to(gpu), dev)
    assert n_pairs == 0 and n_open == P and np.array_equal(src[:, 0], np.arange(P))
    _check_rows(outs, src, none, cloud, "nobody matched")


# ------------------------------------------------------------------------------------------------ end to end
@functools.lru_cache(maxsize=None)
def _doubled():
    """200 well-separated Gaussians, each replaced by two copies at half density, interleaved in random order."""
    rng = np.random.RandomState(5)
    n = 200
    grid = np.stack(np.meshgrid(*[np.arange(6)] * 3, indexing="ij"), -1).reshape(-1, 3)[:n].astype(np.float64)
    xyz = (grid + rng.uniform(-0.2, 0.2, (n, 3))).astype(np.float32)
    _x, density, scaling, rotation = R.random_cloud(n, 6, anisotropy=10.0, scale=0.08)
    order = rng.permutation(2 * n)
    two = [np.concatenate([t, t])[order] for t in (xyz, (density * np.float32(0.5)), scaling, rotation)]
    return (xyz, density, scaling, rotation), two, (order % n)


def test_end_to_end_undoes_a_duplication(gpu):
    from r2_gaussian_amd import merge as MG
    (xyz, density, scaling, rotation), two, origin = _doubled()
    n = len(xyz)
    # the reference alone: the copies cost nothing, every other pair among the 4 nearest neighbours costs more than 1e-6
    from tests import graph_ref as GR
    idx, _d2 = GR.knn_graph(two[0], 4)
    ref_cost = R.edge_costs(idx, *two)
    same = origin[idx] == origin[:, None]
    assert same.sum(1).min() == 1 and ref_cost[same].max() < 1e-9 and ref_cost[~same].min() > 1e-6
    dev = _dev(two, gpu)
    m_xyz, m_density, m_scaling, m_rotation, src, info = MG.merge_gaussians(*dev, max_cost=1e-6, k=4)
    assert info == dict(pairs=n, open=0, P=n) and m_xyz.shape == (n, 3) and m_density.shape == (n, 1)
    src = src.cpu().numpy()
    assert (src[:, 1] >= 0).all() and np.array_equal(origin[src[:, 0]], origin[src[:, 1]])
    o = origin[src[:, 0]]
    got_cov = R.covariance(m_scaling.cpu().numpy().astype(np.float64), m_rotation.cpu().numpy().astype(np.float64))
    want_cov = R.covariance(scaling, rotation)[o]
    cov_err = np.linalg.norm(got_cov - want_cov, axis=(1, 2)) / np.linalg.norm(want_cov, axis=(1, 2))
    got_mass = R.mass(m_density.cpu().numpy(), m_scaling.cpu().numpy())
    want_mass = R.mass(two[1], two[2])
    want_pair = want_mass[src[:, 0]] + want_mass[src[:, 1]]
    mass_err = np.abs(got_mass - want_pair) / want_pair
    x = xyz[o].astype(np.float64)
    print("end to end: covariance %.2f roundings, mass %.2f roundings" % (cov_err.max() / R.U, mass_err.max() / R.U))
    assert (np.abs(m_xyz.cpu().numpy() - x) <= 2 * R.MU_REL * np.abs(x)).all()
    assert (cov_err <= R.COV_REL).all() and (mass_err <= R.MASS_REL).all()
    # total mass before and after
    assert abs(got_mass.sum() - want_mass.sum()) <= R.MASS_REL * want_mass.sum()
    # the same through a graph the caller built, and nothing to merge in the original cloud
    from r2_gaussian_amd import graph as G
    again = MG.merge_gaussians(*dev, max_cost=1e-6, graph=G.knn_graph(dev[0], 4))
    assert all(torch.equal(a, b) for a, b in zip(again[:5], (m_xyz, m_density, m_scaling, m_rotation, torch.as_tensor(src).to(gpu))))
    once = MG.merge_gaussians(*_dev((xyz, density, scaling, rotation), gpu), max_cost=1e-6, k=4)
    assert once[5] == dict(pairs=0, open=0, P=n) and torch.equal(once[0], torch.as_tensor(xyz).to(gpu))


@pytest.mark.parametrize("P", [0, 1, 2])
def test_end_to_end_on_tiny_clouds(gpu, P):
    from r2_gaussian_amd import merge as MG
    dev = _dev(_cloud(P), gpu)
    out = MG.merge_gaussians(*dev, max_cost=np.inf, k=4)
    pairs = P // 2
    assert out[5] == dict(pairs=pairs, open=0, P=P - pairs)
    assert [tuple(t.shape) for t in out[:5]] == [(P - pairs, 3), (P - pairs, 1), (P - pairs, 3), (P - pairs, 4), (P - pairs, 2)]
    if P == 1:
        assert out[4].cpu().tolist() == [[0, -1]] and torch.equal(out[0], dev[0])
    if P == 2:
        assert out[4].cpu().tolist() == [[0, 1]]


def test_max_scale_bounds_the_merged_scales(gpu):
    from r2_gaussian_amd import merge as MG
    P, hi = 1000, 0.125
    dev = _dev(_cloud(P), gpu)
    free = MG.merge_gaussians(*dev, max_cost=np.inf, k=8)
    bound = MG.merge_gaussians(*dev, max_cost=np.inf, k=8, max_scale=hi)
    merged_free, merged_bound = free[4][:, 1] >= 0, bound[4][:, 1] >= 0
    print("largest merged scale: unbounded %.4f, bounded by %.3f: %.4f; pairs %d / %d"
          % (float(free[2][merged_free].max()), hi, float(bound[2][merged_bound].max()), free[5]["pairs"], bound[5]["pairs"]))
    assert float(free[2][merged_free].max()) > hi                  # the bound has something to do
    # (fewer eligible edges need not mean fewer pairs: a greedy matching is not monotone in its edge set)
    assert bound[5]["pairs"] > 100
    assert float(bound[2][merged_bound].max()) <= hi


# ------------------------------------------------------------------------------------------------ the model
def test_model_merge(gpu):
    from r2_gaussian_amd import merge as MG
    from r2_gaussian_amd.gaussians import NAMES, GaussianModel, activate
    _orig, two, _origin = _doubled()
    bound = (0.001, 2.0)
    m = GaussianModel(scale_bound=bound, device=gpu)
    xyz, density, scaling, rotation = _dev(two, gpu)
    lo, hi = bound
    t = (scaling - lo) / (hi - lo)
    m._set(xyz, torch.log(torch.exp(density) - 1), torch.log(t / (1 - t)), rotation)
    m._reset_stats()
    lr = {n: 1e-4 for n in NAMES}

    def step():
        loss = sum((a * a).sum() for a in m.activated())
        loss.backward()
        m.step(lr=lr)

    step(); step()
    P = m.P
    act = [a.detach().clone() for a in m.activated()]
    raw = {n: m._raw[n].detach().clone() for n in NAMES}
    mom = {n: (m.exp_avg[n].clone(), m.exp_avg_sq[n].clone()) for n in NAMES}
    assert all(float(mom[n][0].abs().min()) > 0 for n in ("xyz", "density", "scaling"))
    steps = dict(m.steps)
    # every pair of copies took the same two steps: they still cost (almost) nothing to merge; the rest stays apart
    expected = MG.merge_gaussians(*act, max_cost=1e-5, k=4, rounds=12, max_scale=hi)
    src, info = expected[4], expected[5]
    assert info["pairs"] == P // 2
    pairs = m.merge(1e-5, k=4)
    assert pairs == P // 2 and m.P == P - pairs and m.steps == steps
    d, s, r = activate(m._raw["density"], m._raw["scaling"], m._raw["rotation"], bound)
    assert torch.equal(m.get_density, d) and torch.equal(m.get_scaling, s) and torch.equal(m.get_rotation, r)
    assert all(a.requires_grad and a.is_leaf for a in m.activated())
    # the activations of a merged row are the emitted ones up to the round trip through the inverse activation
    assert torch.allclose(m.get_scaling, expected[2], rtol=1e-4, atol=0)
    assert torch.allclose(m.get_density, expected[1], rtol=1e-4, atol=0)
    assert torch.equal(m.get_xyz.detach(), expected[0])
    for n in NAMES:
        assert float(m.exp_avg[n].abs().max()) == 0 and float(m.exp_avg_sq[n].abs().max()) == 0
    assert m.max_radii2D.shape == (m.P,) and m.xyz_gradient_accum.shape == (m.P, 1) and m.denom.shape == (m.P, 1)
    assert float(m.denom.abs().max()) == 0
    step()
    assert m.steps == {n: steps[n] + 1 for n in NAMES}
    assert all(bool(torch.isfinite(a).all()) for a in m.activated())

    # survivors: a cloud of which only the first 100 rows have their copy's partner nearby
    m2 = GaussianModel(scale_bound=bound, device=gpu)
    far = xyz.clone()
    far[100:] += 20.0 * torch.arange(1, far.shape[0] - 99, device=gpu, dtype=torch.float32)[:, None]
    m2._set(far, raw["density"], raw["scaling"], raw["rotation"], moments=mom, steps=steps)
    m2._reset_stats()
    act2 = [a.detach().clone() for a in m2.activated()]
    exp2 = MG.merge_gaussians(*act2, max_cost=1e-5, k=4, max_scale=hi)
    src2 = exp2[4]
    single = (src2[:, 1] < 0)
    assert 0 < exp2[5]["pairs"] < P // 2 and int(single.sum()) > 0
    assert m2.merge(1e-5, k=4) == exp2[5]["pairs"]
    keep = src2[:, 0].long()
    raw2 = {"xyz": far, "density": raw["density"], "scaling": raw["scaling"], "rotation": raw["rotation"]}
    for n in NAMES:
        assert torch.equal(m2._raw[n].detach()[single], raw2[n][keep][single]), n           # survivors: their own raw bits
        assert torch.equal(m2.exp_avg[n][single], mom[n][0][keep][single]), n               # ... and their own moments
        assert torch.equal(m2.exp_avg_sq[n][single], mom[n][1][keep][single]), n
        assert float(m2.exp_avg[n][~single].abs().max()) == 0 and float(m2.exp_avg_sq[n][~single].abs().max()) == 0
    for a, e in zip(m2.activated()[1:], exp2[1:4]):
        assert torch.equal(a.detach()[single], e[single])                                  # activations of survivors: unchanged bits
    assert m2.steps == steps and m2.denom.shape == (m2.P, 1)
    # fewer than two Gaussians: nothing happens
    empty = GaussianModel(scale_bound=bound, device=gpu)
    assert empty.merge(1.0) == 0 and empty.P == 0
