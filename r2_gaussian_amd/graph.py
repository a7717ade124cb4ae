"""Neighbour graphs of a point cloud and a smoothness loss over their edges (include/r2hip.h: r2_knn_graph,
r2_graph_transpose, r2_graph_loss, r2_graph_loss_backward).  No counterpart in the reference.

    g = knn_graph(xyz, 8)                      # idx, dist2 [P, 8] and the incoming edges of every node
    loss = graph_smoothness(density[:, 0], g)  # mean |v_i - v_j| over the edges, one autograd node

The loss is differentiable in ``values`` only: the graph and the weights are structure (as the culling is in the exact
operators), so rebuild the graph from ``xyz.detach()`` whenever the cloud has moved enough.
"""
import torch

from . import _lib
from ._boundary import _F32, call, require_gpu, workspace

_I32 = torch.int32
KINDS = {"l1": _lib.R2_GRAPH_KIND_L1, "l2": _lib.R2_GRAPH_KIND_L2, "huber": _lib.R2_GRAPH_KIND_HUBER}


class NeighbourGraph:
    """idx [P, K] int32 (-1 = no edge), dist2 [P, K] float32 or None, in_offsets [P + 1] / in_edges [P * K] int32: the valid
    edges e = i * K + k pointing at node j are in_edges[in_offsets[j]:in_offsets[j + 1]], ascending.  n_edges: valid edges."""

    __slots__ = ("idx", "dist2", "in_offsets", "in_edges", "P", "K", "n_edges")

    def __init__(self, idx, dist2, in_offsets, in_edges, n_edges):
        self.idx, self.dist2, self.in_offsets, self.in_edges = idx, dist2, in_offsets, in_edges
        self.P, self.K = int(idx.shape[0]), int(idx.shape[1])
        self.n_edges = int(n_edges)


def _transpose(idx):
    P, K = idx.shape
    dev = idx.device
    in_offsets = torch.empty((P + 1,), dtype=_I32, device=dev)
    in_edges = torch.empty((P * K,), dtype=_I32, device=dev)
    nbytes = int(_lib.lib().r2_graph_transpose_workspace_bytes(P, K))
    ws = workspace(nbytes, dev)
    call("r2_graph_transpose", dev, P, K, idx if P else None, in_offsets, in_edges if P else None, ws if nbytes else None, nbytes)
    return in_offsets, in_edges


def knn_graph(xyz, k):
    """The k nearest neighbours of every point of xyz [P, 3] (float32 on the GPU), ordered by (squared distance, index), self
    excluded by index, and the transposed graph, built on the tensor's device and current stream.  Rows of fewer than k
    neighbours (P - 1 < k) end in idx = -1, dist2 = +inf.  1 <= k <= 16."""
    require_gpu(xyz, "xyz")
    if xyz.ndim != 2 or xyz.shape[1] != 3:
        raise ValueError("xyz must have dimensions (num_points, 3), got %s" % (tuple(xyz.shape),))
    dev = xyz.device
    pts = xyz.detach().to(_F32).contiguous()
    P, K = int(pts.shape[0]), int(k)
    idx = torch.empty((P, max(K, 0)), dtype=_I32, device=dev)
    dist2 = torch.empty((P, max(K, 0)), dtype=_F32, device=dev)
    # the library does not allocate: the grid search's workspace comes from torch's allocator
    nbytes = int(_lib.lib().r2_knn_graph_workspace_bytes(P, K))
    ws = workspace(nbytes, dev)
    call("r2_knn_graph", dev, P, pts if P else None, K, idx if P else None, dist2 if P else None, ws if nbytes else None, nbytes)
    in_offsets, in_edges = _transpose(idx)
    return NeighbourGraph(idx, dist2, in_offsets, in_edges, P * min(K, max(P - 1, 0)))


def graph_from_indices(idx):
    """A caller-made graph: idx [P, K] integer tensor on the GPU, row i = the targets of node i's edges, anything outside [0, P)
    = no edge.  Transpose only (dist2 = None).  Reads the number of valid edges back from in_offsets[P]: one host read."""
    require_gpu(idx, "idx")
    if idx.ndim != 2 or idx.shape[1] < 1:
        raise ValueError("idx must have dimensions (num_points, K >= 1), got %s" % (tuple(idx.shape),))
    idx = idx.to(_I32).contiguous()
    in_offsets, in_edges = _transpose(idx)
    return NeighbourGraph(idx, None, in_offsets, in_edges, int(in_offsets[-1].item()))


def edge_weights(graph, bandwidth=None):
    """w [P, K] = exp(-dist2 / (2 h^2)), 0 on missing edges: h = bandwidth, or per row h^2 = the mean of the row's finite dist2.
    Plain torch, not differentiated."""
    if graph.dist2 is None:
        raise ValueError("edge_weights needs a graph with distances (knn_graph)")
    with torch.no_grad():
        d2 = graph.dist2
        finite = torch.isfinite(d2) & (graph.idx >= 0)
        d2z = torch.where(finite, d2, torch.zeros_like(d2))
        if bandwidth is None:
            h2 = d2z.sum(1, keepdim=True) / finite.sum(1, keepdim=True).clamp(min=1)
        else:
            h2 = torch.full((graph.P, 1), float(bandwidth) ** 2, dtype=_F32, device=d2.device)
        w = torch.exp(-d2z / (2 * h2).clamp(min=torch.finfo(_F32).tiny))
        return torch.where(finite, w, torch.zeros_like(w)).contiguous()


class _GraphSmoothness(torch.autograd.Function):
    @staticmethod
    def forward(ctx, values, graph, weights, kind, delta, scale):
        v = values.detach().to(_F32).contiguous().view(-1)
        dev = v.device
        P, K = graph.P, graph.K
        scratch = torch.empty(int(_lib.lib().r2_graph_loss_scratch_floats(P, K)), dtype=_F32, device=dev)
        loss = torch.empty(1, dtype=_F32, device=dev)
        call("r2_graph_loss", dev, P, K, v if P else None, graph.idx if P else None, weights if P else None, kind, delta, scale,
             scratch, loss)
        ctx.save_for_backward(v)
        ctx.graph, ctx.weights, ctx.args = graph, weights, (kind, delta, scale)
        ctx.shape, ctx.dtype = values.shape, values.dtype
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        (v,) = ctx.saved_tensors
        graph, w = ctx.graph, ctx.weights
        kind, delta, scale = ctx.args
        P, K = graph.P, graph.K
        dev = v.device
        grad = torch.empty(P, dtype=_F32, device=dev)
        if P:
            gd = g.detach().to(_F32).contiguous().view(1)
            call("r2_graph_loss_backward", dev, P, K, v, graph.idx, w, graph.in_offsets, graph.in_edges, kind, delta, scale, gd, grad)
        return grad.view(ctx.shape).to(ctx.dtype), None, None, None, None, None


def graph_smoothness(values, graph, weights=None, kind="l1", delta=None, reduction="mean"):
    """scale * sum over the graph's edges (i -> j) of w_ij * phi(values[i] - values[j]) as one autograd node, differentiable
    in ``values`` ([P] or [P, 1]) only.  kind: "l1" |x|, "l2" x^2, "huber" (needs delta > 0).  weights: None (1) or [P, K]
    non-negative (edge_weights).  reduction: "mean" (scale = 1 / max(valid edges, 1)) or "sum".  Shapes that disagree with
    the graph raise ValueError."""
    require_gpu(values, "values")
    if kind not in KINDS:
        raise ValueError("kind must be one of %s, got %r" % (sorted(KINDS), kind))
    if reduction not in ("mean", "sum"):
        raise ValueError("reduction must be 'mean' or 'sum', got %r" % (reduction,))
    if kind == "huber" and not (delta is not None and float(delta) > 0):
        raise ValueError("kind 'huber' needs delta > 0, got %r" % (delta,))
    if not (values.ndim == 1 or (values.ndim == 2 and values.shape[1] == 1)) or values.shape[0] != graph.P:
        raise ValueError("values must be [P] or [P, 1] with the graph's P = %d, got %s" % (graph.P, tuple(values.shape)))
    if values.device != graph.idx.device:
        raise ValueError("values and graph live on different devices")
    if weights is not None:
        if tuple(weights.shape) != (graph.P, graph.K) or weights.device != values.device:
            raise ValueError("weights must be [P, K] = [%d, %d] on the graph's device, got %s" % (graph.P, graph.K, tuple(weights.shape)))
        weights = weights.detach().to(_F32).contiguous()
    scale = 1.0 / max(graph.n_edges, 1) if reduction == "mean" else 1.0
    return _GraphSmoothness.apply(values, graph, weights, KINDS[kind], float(delta) if delta is not None else 0.0, float(scale))
