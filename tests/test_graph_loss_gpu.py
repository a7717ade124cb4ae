"""GPU: r2_graph_transpose (exact), r2_graph_loss and r2_graph_loss_backward against the float64 reference of
tests/graph_ref.py under bounds made of float32 roundings counted along the kernels' fixed summation orders
(include/r2hip.h), and the Python surface graph.graph_smoothness on top of them."""
import functools

import numpy as np
import pytest
import torch

from r2_gaussian_amd import scene as S
from r2_gaussian_amd._lib import R2_GRAPH_LOSS_CHAIN, R2_GRAPH_LOSS_HUB
from tests import graph_ref as R

pytestmark = pytest.mark.gpu
U = 2.0 ** -24   # unit roundoff of float32
DELTA = 0.5
GRAPHS = ("knn-257x8", "knn-65x3", "holes", "out-of-range", "star")


@functools.lru_cache(maxsize=None)
def _graph(name):
    """idx [P, K] int32 (numpy) of the named graph."""
    rng = np.random.RandomState(5)
    if name.startswith("knn-"):
        P, K = (int(t) for t in name[4:].split("x"))
        return R.knn_graph(S.make_cloud(P, seed=P).xyz.numpy(), K)[0]
    if name == "holes":          # -1 slots scattered through the rows, whole rows without edges, nodes nobody points at
        idx = rng.randint(0, 60, size=(100, 5)).astype(np.int32)
        idx[rng.rand(100, 5) < 0.3] = -1
        idx[10] = -1
        idx[77] = -1
        return idx
    if name == "out-of-range":   # targets outside [-1, P) are no edges either
        idx = rng.randint(0, 40, size=(40, 4)).astype(np.int32)
        idx[3, 1], idx[7, 0], idx[39, 3], idx[20, 2] = 40, 1000, -5, np.iinfo(np.int32).max
        return idx
    if name == "star":           # everybody points at node 0: in-degree 299, beyond the wave-sum threshold
        idx = np.zeros((300, 1), dtype=np.int32)
        idx[0, 0] = -1
        return idx
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def _values(P):
    rng = np.random.RandomState(P)
    v = rng.randn(P).astype(np.float32)
    v[::3] = np.round(v[::3] * 2) / 2   # ties and exact differences among a third of the nodes
    return v


def _weights(idx):
    return np.random.RandomState(9).rand(*idx.shape).astype(np.float32)


def _transpose_gpu(idx, gpu):
    from r2_gaussian_amd import graph as G
    g = G.graph_from_indices(torch.from_numpy(idx).to(gpu))
    return g, g.in_offsets.cpu().numpy(), g.in_edges.cpu().numpy()


@pytest.mark.parametrize("name", GRAPHS)
def test_transpose(name, gpu):
    idx = _graph(name)
    off, edges = R.transpose(idx)
    g, goff, gedges = _transpose_gpu(idx, gpu)
    assert goff.dtype == np.int32 and np.array_equal(goff, off)
    assert np.array_equal(gedges[:off[-1]], edges) and g.n_edges == off[-1]
    if name == "star":
        assert off[1] - off[0] == 299 > R2_GRAPH_LOSS_HUB
    g2, goff2, gedges2 = _transpose_gpu(idx, gpu)
    assert np.array_equal(goff2, goff) and np.array_equal(gedges2[:off[-1]], gedges[:off[-1]])


def test_transpose_tiny(gpu):
    for idx in (np.zeros((0, 3), dtype=np.int32), np.full((1, 3), -1, dtype=np.int32), np.zeros((1, 2), dtype=np.int32)):
        off, edges = R.transpose(idx)
        g, goff, gedges = _transpose_gpu(idx, gpu)
        assert np.array_equal(goff, off) and np.array_equal(gedges[:off[-1]], edges)
    # a power of two of nodes: the key of an invalid edge (P) needs one bit more than the largest target
    idx = np.arange(64, dtype=np.int32).reshape(64, 1)[::-1].copy()
    idx[5] = -1
    off, edges = R.transpose(idx)
    g, goff, gedges = _transpose_gpu(idx, gpu)
    assert np.array_equal(goff, off) and np.array_equal(gedges[:off[-1]], edges)


def _raw(idx, v, w, kind, scale, g, gpu):
    """r2_graph_loss and r2_graph_loss_backward through the C ABI -> (loss float32, grad [P] float32)."""
    from r2_gaussian_amd import _lib
    from r2_gaussian_amd._C import _stream
    L = _lib.lib()
    P, K = idx.shape
    gr, _, _ = _transpose_gpu(idx, gpu)
    dv = torch.from_numpy(v).to(gpu)
    dw = torch.from_numpy(w).to(gpu) if w is not None else None
    scratch = torch.empty(int(L.r2_graph_loss_scratch_floats(P, K)), dtype=torch.float32, device=gpu)
    loss = torch.full((1,), float("nan"), dtype=torch.float32, device=gpu)
    grad = torch.full((P,), float("nan"), dtype=torch.float32, device=gpu)
    dg = torch.tensor([g], dtype=torch.float32, device=gpu)
    args = (P, K, dv.data_ptr(), gr.idx.data_ptr(), dw.data_ptr() if dw is not None else None)
    rc = L.r2_graph_loss(*args, kind, DELTA, scale, scratch.data_ptr(), loss.data_ptr(), _stream(gpu))
    assert rc == 0, L.r2_last_error()
    rc = L.r2_graph_loss_backward(*args, gr.in_offsets.data_ptr(), gr.in_edges.data_ptr(), kind, DELTA, scale, dg.data_ptr(),
                                  grad.data_ptr(), _stream(gpu))
    assert rc == 0, L.r2_last_error()
    torch.cuda.synchronize()
    return loss.cpu().numpy()[0], grad.cpu().numpy()


def _check(idx, v, w, kind, scale, g, got_loss, got_grad):
    """The bounds of the issue, (c + 4) u and (K + indegree + 4) u, counted in roundings u = 2^-24 relative to a term.
    Forward: a term carries at most 5 (Huber's linear branch: the difference, which |x| - delta / 2 >= |x| / 2 at most
    doubles, that subtraction, the product with delta, the weight; 4 for x * x, 2 for |x|); on its way to the result it meets
    at most c - 1 more, because c = R2_GRAPH_LOSS_CHAIN counts the thread's first addition 0 + t, which is exact.
    Backward: 2 in a term (difference, weight), at most K + indegree additions, 2 for g * scale and its product."""
    scale = float(np.float32(scale))
    ref = R.loss_and_grad(v, idx, w, kind, DELTA, scale, g=float(np.float32(g)))
    K = idx.shape[1]
    tol = (R2_GRAPH_LOSS_CHAIN + 4) * U * scale * ref["abs_sum"]
    err = abs(float(got_loss) - ref["loss"])
    print("kind %d loss %.9g ref %.9g err %.3g bound %.3g" % (kind, got_loss, ref["loss"], err, tol))
    assert err <= tol
    gtol = (K + ref["indegree"] + 4) * U * abs(float(np.float32(g))) * scale * ref["abs_terms"]
    gerr = np.abs(got_grad.astype(np.float64) - ref["grad"])
    worst = int(np.argmax(gerr - gtol)) if gerr.size else -1
    if worst >= 0:
        print("grad: worst node %d err %.3g bound %.3g" % (worst, gerr[worst], gtol[worst]))
    assert np.all(gerr <= gtol)
    lonely = (ref["indegree"] == 0) & (ref["outdegree"] == 0)
    assert np.all(got_grad[lonely] == 0) and not np.any(np.signbit(got_grad[lonely]))
    return ref


@pytest.mark.parametrize("weighted", (False, True), ids=("unit", "weighted"))
@pytest.mark.parametrize("kind", (0, 1, 2), ids=("l1", "l2", "huber"))
@pytest.mark.parametrize("name", GRAPHS)
def test_forward_and_backward(name, kind, weighted, gpu):
    idx = _graph(name)
    v = _values(idx.shape[0])
    w = _weights(idx) if weighted else None
    scale, g = 1.0 / 37.0, -2.5   # an upstream gradient other than 1
    loss, grad = _raw(idx, v, w, kind, scale, g, gpu)
    ref = _check(idx, v, w, kind, scale, g, loss, grad)
    if name == "holes":
        assert ((ref["indegree"] == 0) & (ref["outdegree"] == 0)).sum() >= 2
    loss2, grad2 = _raw(idx, v, w, kind, scale, g, gpu)   # the same bits on every call
    assert np.array_equal(np.float32(loss).view(np.uint32), np.float32(loss2).view(np.uint32))
    assert np.array_equal(grad.view(np.uint32), grad2.view(np.uint32))


def test_tied_values_have_no_l1_gradient(gpu):
    idx = _graph("knn-257x8")
    v = np.full(257, 0.3, dtype=np.float32)
    loss, grad = _raw(idx, v, None, 0, 1.0, 1.0, gpu)
    assert loss == 0 and np.all(grad == 0)
    # two plateaus: only the edges across the step contribute, each exactly +-w
    v[:100] = 1.3
    w = _weights(idx)
    loss, grad = _raw(idx, v, w, 0, 1.0, 1.0, gpu)
    _check(idx, v, w, 0, 1.0, 1.0, loss, grad)
    cross = (v[:, None] != v[idx])
    assert np.all(grad[~cross.any(1) & ~np.isin(np.arange(257), idx[cross])] == 0)


def test_empty_graph(gpu):
    from r2_gaussian_amd import graph as G
    g = G.graph_from_indices(torch.zeros((0, 3), dtype=torch.int32, device=gpu))
    v = torch.zeros(0, device=gpu, requires_grad=True)
    loss = G.graph_smoothness(v, g)
    assert loss.item() == 0.0
    loss.backward()
    assert v.grad.shape == (0,)


@pytest.mark.parametrize("kind", ("l1", "l2", "huber"))
def test_graph_smoothness_autograd(kind, gpu):
    """gradcheck does not apply in float32: the autograd node's gradient against the float64 reference under the bound."""
    from r2_gaussian_amd import graph as G
    pts = S.make_cloud(257, seed=257).xyz
    g = G.knn_graph(pts.to(gpu), 8)
    idx = _graph("knn-257x8")
    assert np.array_equal(g.idx.cpu().numpy(), idx)
    v = _values(257)
    w = G.edge_weights(g)
    x = torch.from_numpy(v).to(gpu).view(-1, 1).requires_grad_(True)   # [P, 1] like a density column
    loss = G.graph_smoothness(x, g, weights=w, kind=kind, delta=DELTA if kind == "huber" else None)
    (3.0 * loss).backward()
    assert x.grad.shape == (257, 1) and loss.ndim == 0
    _check(idx, v, w.cpu().numpy(), G.KINDS[kind], 1.0 / (257 * 8), 3.0, loss.item(), x.grad[:, 0].cpu().numpy())
    # reduction "sum", no weights, [P]
    y = torch.from_numpy(v).to(gpu).requires_grad_(True)
    loss = G.graph_smoothness(y, g, kind=kind, delta=DELTA if kind == "huber" else None, reduction="sum")
    loss.backward()
    _check(idx, v, None, G.KINDS[kind], 1.0, 1.0, loss.item(), y.grad.cpu().numpy())


def test_mean_uses_the_valid_edge_count(gpu):
    from r2_gaussian_amd import graph as G
    idx = _graph("holes")
    g = G.graph_from_indices(torch.from_numpy(idx).to(gpu))
    E = int((idx >= 0).sum())
    assert g.n_edges == E and g.dist2 is None
    v = _values(100)
    x = torch.from_numpy(v).to(gpu).requires_grad_(True)
    loss = G.graph_smoothness(x, g, kind="l2")
    loss.backward()
    _check(idx, v, None, 1, 1.0 / E, 1.0, loss.item(), x.grad.cpu().numpy())
    # a k-NN graph with short rows: P * min(K, P - 1) edges
    g3 = G.knn_graph(S.make_cloud(3, seed=1).xyz.to(gpu), 8)
    x3 = torch.tensor([0.0, 1.0, 3.0], device=gpu)
    assert G.graph_smoothness(x3, g3).item() == pytest.approx((1 + 3 + 1 + 2 + 3 + 2) / 6.0, rel=1e-6)


def test_shape_errors(gpu):
    from r2_gaussian_amd import _lib
    from r2_gaussian_amd import graph as G
    g = G.graph_from_indices(torch.from_numpy(_graph("holes")).to(gpu))
    with pytest.raises(ValueError, match="P = 100"):
        G.graph_smoothness(torch.zeros(99, device=gpu), g)
    with pytest.raises(ValueError):
        G.graph_smoothness(torch.zeros(100, 2, device=gpu), g)
    with pytest.raises(ValueError):
        G.graph_smoothness(torch.zeros(100, device=gpu), g, weights=torch.ones(100, 4, device=gpu))
    with pytest.raises(ValueError):
        G.graph_smoothness(torch.zeros(100, device=gpu), g, kind="huber")
    with pytest.raises(ValueError):
        G.graph_smoothness(torch.zeros(100, device=gpu), g, kind="l3")
    with pytest.raises(ValueError):
        G.edge_weights(g)
    with pytest.raises(_lib.R2HipError, match="GPU tensor"):
        G.graph_smoothness(torch.zeros(100), g)
    L = _lib.lib()
    one = torch.zeros(4, device=gpu)
    assert L.r2_graph_loss(1, 1, one.data_ptr(), one.data_ptr(), None, 3, 0.0, 1.0, one.data_ptr(), one.data_ptr(), None) == _lib.R2_ERR_INVALID
    assert b"kind 3" in L.r2_last_error()
    assert L.r2_graph_loss(1, 1, one.data_ptr(), one.data_ptr(), None, 2, 0.0, 1.0, one.data_ptr(), one.data_ptr(), None) == _lib.R2_ERR_INVALID
    assert b"delta > 0" in L.r2_last_error()
