"""GPU: r2_knn_graph against the brute-force float32 reference of tests/graph_ref.py, bit for bit in idx AND dist2 -- the
contract is a total order (dist2, index) on bit-exact distances, so there is no tolerance -- through the grid search, the
exhaustive search and the hand-overs between them; consistency with distCUDA2; argument errors."""
import functools

import numpy as np
import pytest
import torch

from r2_gaussian_amd import scene as S
from tests import graph_ref as R

pytestmark = pytest.mark.gpu
KS = (1, 3, 8, 16)


def _gpu_graph(pts, K, gpu, workspace=True, stream=None):
    """The raw entry point: with the workspace the grid search may run, without it the exhaustive kernel does."""
    from r2_gaussian_amd import _lib
    from r2_gaussian_amd._C import _stream
    L = _lib.lib()
    P = pts.shape[0]
    dp = pts.to(gpu).contiguous()
    idx = torch.full((P, K), -7, dtype=torch.int32, device=gpu)
    d2 = torch.full((P, K), -7.0, dtype=torch.float32, device=gpu)
    nbytes = int(L.r2_knn_graph_workspace_bytes(P, K)) if workspace else 0
    ws = torch.empty((max(nbytes, 1),), dtype=torch.uint8, device=gpu)
    rc = L.r2_knn_graph(P, dp.data_ptr() if P else None, K, idx.data_ptr() if P else None, d2.data_ptr() if P else None,
                        ws.data_ptr() if nbytes else None, nbytes, stream if stream is not None else _stream(gpu))
    assert rc == 0, L.r2_last_error()
    torch.cuda.synchronize()
    return idx.cpu().numpy(), d2.cpu().numpy()


def _same(got, ref):
    return np.array_equal(got[0], ref[0]) and np.array_equal(got[1].view(np.uint32), ref[1].view(np.uint32))


@functools.lru_cache(maxsize=None)
def _random_cloud(P):
    return S.make_cloud(P, seed=100 + P).xyz.contiguous() if P else torch.zeros((0, 3))


@functools.lru_cache(maxsize=None)
def _reference16(name):
    """(points, reference for K = 16), computed once per cloud: the first K columns are the reference for every K <= 16 (the
    first K of a total order are a prefix of the first 16)."""
    pts = _random_cloud(int(name)) if name.isdigit() else _stress_cloud(name)
    return pts, R.knn_graph(pts.numpy(), 16)


def _ref(name, K):
    pts, (idx, d2) = _reference16(name)
    return pts, (idx[:, :K], d2[:, :K])


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("P", ["0", "1", "2", "K", "K+1", "63", "64", "65", "255", "256", "257", "4095", "4096", "4097"])
def test_random_clouds(P, K, gpu):
    """P straddles the wave, the workgroup and the grid threshold; rows of fewer than K neighbours end in -1 / +inf."""
    n = K if P == "K" else K + 1 if P == "K+1" else int(P)
    pts, ref = _ref(str(n), K)
    got = _gpu_graph(pts, K, gpu)
    assert _same(got, ref)
    if n - 1 < K:
        have = max(n - 1, 0)
        assert np.all(got[0][:, have:] == -1) and np.all(np.isposinf(got[1][:, have:]))
        assert np.all(got[0][:, :have] >= 0)


STRESS = ("lattice", "duplicates", "collinear", "clustered", "translated", "elongated")


def _stress_cloud(name):
    g = torch.Generator().manual_seed(17)
    if name == "lattice":       # 17^3 integer lattice: 6 neighbours at distance^2 1, 12 at 2, 8 at 3 -- K = 8 and 16 cut inside a tie group
        a = torch.arange(17, dtype=torch.float32)
        pts = torch.stack(torch.meshgrid(a, a, a, indexing="ij"), -1).reshape(-1, 3)
        pts = pts[torch.randperm(pts.shape[0], generator=g)]   # (so that index order is not lattice order)
    elif name == "duplicates":  # 300 copies of one point among 4000 others
        pts = torch.cat([torch.rand(4000, 3, generator=g) * 2 - 1, torch.tensor([[0.25, -0.5, 0.125]]).repeat(300, 1)])
        pts = pts[torch.randperm(pts.shape[0], generator=g)]
    elif name == "collinear":
        pts = torch.zeros(4200, 3)
        pts[:, 0] = torch.rand(4200, generator=g)
    elif name == "clustered":   # 4000 points inside one cell: handed over to the exhaustive kernel
        pts = torch.cat([torch.randn(4000, 3, generator=g) * 1e-5 + 0.3, torch.rand(800, 3, generator=g) * 2 - 1])
    elif name == "translated":
        pts = S.make_cloud(4500, seed=8).xyz + torch.tensor([1000.0, -1000.0, 1000.0])
    else:                       # several hundred cells along one axis
        pts = torch.rand(5000, 3, generator=g) * torch.tensor([400.0, 1.0, 1.0]) + torch.tensor([30.0, 0.0, -3.0])
    return pts.contiguous()


@pytest.mark.parametrize("K", (3, 8, 16))
@pytest.mark.parametrize("name", STRESS)
def test_clouds_that_stress_the_search(name, K, gpu):
    pts, ref = _ref(name, K)
    assert pts.shape[0] >= 4096
    grid = _gpu_graph(pts, K, gpu)
    assert _same(grid, ref), "with workspace"
    # the exhaustive search (no workspace) gives the same bits as the grid search
    assert _same(_gpu_graph(pts, K, gpu, workspace=False), grid), "grid against exhaustive"
    if name == "lattice":
        d = ref[1]
        inner = np.all((pts.numpy() >= 1) & (pts.numpy() <= 15), axis=1)
        assert np.all(d[inner, :min(K, 6)] == 1) and (K < 8 or np.all(d[inner, 6:min(K, 18)] == 2))


@pytest.mark.parametrize("P", (4096, 4097))
def test_same_bits_from_both_searches_twice_and_on_a_stream(P, gpu):
    K = 8
    pts, ref = _ref(str(P), K)
    a = _gpu_graph(pts, K, gpu)
    assert _same(_gpu_graph(pts, K, gpu, workspace=False), a)
    assert _same(_gpu_graph(pts, K, gpu), a)
    s = torch.cuda.Stream(device=gpu)
    with torch.cuda.stream(s):
        b = _gpu_graph(pts, K, gpu, stream=s.cuda_stream)
    assert _same(b, ref)


@pytest.mark.parametrize("name", ("4", "65", "4097", "lattice", "duplicates", "translated"))
def test_consistent_with_distCUDA2(name, gpu):
    """((d0 + d1) + d2) / 3 in float32 over the three nearest is distCUDA2's value, bit for bit (knn.hip sums b0 <= b1 <= b2 in
    that order)."""
    from r2_gaussian_amd import distCUDA2
    from r2_gaussian_amd import graph as G
    pts = _reference16(name)[0].to(gpu)
    want = distCUDA2(pts).cpu().numpy()
    for K in (3, 8):
        d = G.knn_graph(pts, K).dist2.cpu().numpy()
        # in numpy: a correctly rounded float32 division (torch divides a GPU tensor by a scalar through its reciprocal)
        got = ((d[:, 0] + d[:, 1]) + d[:, 2]) / np.float32(3.0)
        assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32)), K


def test_python_surface(gpu):
    from r2_gaussian_amd import graph as G
    pts, ref = _ref("257", 8)
    g = G.knn_graph(pts.to(gpu), 8)
    assert (g.P, g.K, g.n_edges) == (257, 8, 257 * 8)
    assert g.idx.dtype == torch.int32 and g.dist2.dtype == torch.float32 and g.idx.shape == (257, 8)
    assert np.array_equal(g.idx.cpu().numpy(), ref[0]) and np.array_equal(g.dist2.cpu().numpy(), ref[1])
    off, edges = R.transpose(ref[0])
    assert np.array_equal(g.in_offsets.cpu().numpy(), off) and np.array_equal(g.in_edges.cpu().numpy()[:off[-1]], edges)
    small = G.knn_graph(pts[:3].to(gpu), 8)
    assert small.n_edges == 6 and int(small.in_offsets[-1]) == 6
    empty = G.knn_graph(torch.zeros((0, 3), device=gpu), 3)
    assert empty.P == 0 and empty.n_edges == 0 and empty.in_offsets.cpu().tolist() == [0]
    w = G.edge_weights(g)
    d2 = torch.from_numpy(ref[1].astype(np.float64))
    want = torch.exp(-d2 / (2 * d2.mean(1, keepdim=True)))
    assert torch.allclose(w.cpu().double(), want, rtol=1e-5, atol=0) and w.shape == (257, 8)
    w = G.edge_weights(small, bandwidth=0.5)
    assert torch.all(w[:, 2:] == 0) and torch.allclose(w[:, :2], torch.exp(-small.dist2[:, :2] / 0.5), rtol=1e-5)


def test_errors(gpu):
    from r2_gaussian_amd import _lib
    from r2_gaussian_amd import graph as G
    pts = _random_cloud(64).to(gpu)
    for K in (0, 17):
        with pytest.raises(_lib.R2HipError, match="r2_knn_graph: K = %d" % K):
            G.knn_graph(pts, K)
        L = _lib.lib()
        idx = torch.empty((64, 17), dtype=torch.int32, device=gpu)
        d2 = torch.empty((64, 17), dtype=torch.float32, device=gpu)
        assert L.r2_knn_graph(64, pts.data_ptr(), K, idx.data_ptr(), d2.data_ptr(), None, 0, None) == _lib.R2_ERR_INVALID
        assert b"outside [1, 16]" in L.r2_last_error()
        assert L.r2_knn_graph(0, None, K, None, None, None, 0, None) == _lib.R2_ERR_INVALID   # K is checked before P = 0
    with pytest.raises(_lib.R2HipError, match="GPU tensor"):
        G.knn_graph(pts.cpu(), 3)
    with pytest.raises(_lib.R2HipError, match="GPU tensor"):
        G.graph_from_indices(torch.zeros((4, 2), dtype=torch.int32))
    with pytest.raises(ValueError):
        G.knn_graph(torch.zeros((5, 2), device=gpu), 3)
