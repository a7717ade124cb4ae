"""Moment-preserving merging of neighbouring Gaussians (include/r2hip.h: r2_merge_cost, r2_graph_match, r2_merge_count,
r2_merge_emit).  No counterpart in the reference, whose density control only grows the cloud or deletes from it.

    xyz, density, scaling, rotation, src, info = merge_gaussians(xyz, density, scaling, rotation, max_cost=0.1)

Candidates are the edges of a neighbour graph (graph.knn_graph); the cost of an edge is Runnalls' Kullback-Leibler bound per
unit mass; a locally-dominant-edge matching picks disjoint pairs in key order (cost, then the pair's indices), which at
convergence is the sequential greedy matching; each pair becomes the one Gaussian of the same mass, mean and second moment.
All parameters are ACTIVATED ones.  Nothing here is differentiated.  One host read per merge (the number of pairs).
"""
import ctypes as C
import math

import numpy as np
import torch

from . import _lib
from ._boundary import _F32, WIDTHS, call, cloud_checked, require_gpu, workspace
from .graph import NeighbourGraph, knn_graph

_I32 = torch.int32


def _check_graph(graph):
    if not isinstance(graph, NeighbourGraph):
        raise ValueError("graph must be a graph.NeighbourGraph (knn_graph, graph_from_indices), got %r" % (type(graph).__name__,))
    return graph.idx.device


def _params(graph, xyz, density, scaling, rotation):
    """The four activated tensors as contiguous float32 on the graph's device; density may be [P] or [P, 1]."""
    dev = _check_graph(graph)
    return cloud_checked((xyz, density, scaling, rotation), graph.P, dev)


def _edge_array(graph, t, name, dtype):
    require_gpu(t, name)
    if tuple(t.shape) != (graph.P, graph.K) or t.device != graph.idx.device:
        raise ValueError("%s must be [P, K] = [%d, %d] on the graph's device, got %s" % (name, graph.P, graph.K, tuple(t.shape)))
    return t.detach().to(dtype).contiguous()


def _node_array(graph, t, name):
    require_gpu(t, name)
    if tuple(t.shape) != (graph.P,) or t.device != graph.idx.device:
        raise ValueError("%s must be [P] = [%d] on the graph's device, got %s" % (name, graph.P, tuple(t.shape)))
    return t.detach().to(_I32).contiguous()


def max_trace_of(max_scale):
    """The largest float32 that does not exceed max_scale^2 (the cost kernel's trace bound), 0 = no bound for None."""
    if max_scale is None:
        return 0.0
    hi = float(max_scale)
    if not hi > 0 or not math.isfinite(hi):
        raise ValueError("max_scale must be a positive finite number or None, got %r" % (max_scale,))
    t = np.float32(hi * hi)
    if float(t) > hi * hi:
        t = np.nextafter(t, np.float32(0))
    return float(t)


def merge_costs(graph, xyz, density, scaling, rotation, max_scale=None):
    """cost [P, K] float32 of merging the two ends of every edge: max(0, 1/2 [log det S_ab - a log det S_a - (1 - a) log det S_b])
    with a = m_a / (m_a + m_b), m = density * s1 s2 s3; +inf on missing and self edges, on non-positive or non-finite
    parameters, and, with max_scale, where trace S_ab > max_scale^2 (no merged scale then exceeds max_scale).  Both directions
    of a pair carry the same bits."""
    p = _params(graph, xyz, density, scaling, rotation)
    max_trace = max_trace_of(max_scale)
    dev, P, K = graph.idx.device, graph.P, graph.K
    cost = torch.empty((P, K), dtype=_F32, device=dev)
    if P:
        call("r2_merge_cost", dev, P, K, graph.idx, *p, max_trace, cost)
    return cost


def match_edges(graph, cost, max_cost, rounds=12):
    """mate [P] int32 (partner or -1) after `rounds` rounds of the locally-dominant-edge rule on the edges with
    cost <= max_cost; the key of an edge is (cost, min(i, j), max(i, j)).  Any graph, any float costs.  No host read: whether the
    matching is maximal is merge_pairs' info["open"] == 0."""
    _check_graph(graph)
    cost = _edge_array(graph, cost, "cost", _F32)
    rounds = int(rounds)
    if rounds < 0:
        raise ValueError("rounds must be >= 0, got %r" % (rounds,))
    dev, P, K = graph.idx.device, graph.P, graph.K
    mate = torch.empty((P,), dtype=_I32, device=dev)
    if P:
        nbytes = int(_lib.lib().r2_graph_match_workspace_bytes(P))
        ws = workspace(nbytes, dev)
        call("r2_graph_match", dev, P, K, graph.idx, graph.in_offsets, graph.in_edges, cost, float(max_cost), rounds, mate, ws, nbytes)
    return mate


def merge_pairs(graph, cost, max_cost, mate, xyz, density, scaling, rotation):
    """Replace every matched pair by its moment-matched Gaussian.  -> (xyz, density [Pn, 1], scaling, rotation, src, info):
    Pn = P - pairs rows in ascending order of the original index, a pair at its lower index; src [Pn, 2] int32 = (a, b), b = -1
    for an unmerged row, which is a bit copy; info = dict(pairs, open, P = Pn), open = unmatched nodes that still have an edge
    with cost <= max_cost to an unmatched node (0: the matching is maximal).  Entries of mate that are no valid pairing count
    as -1.  One host read."""
    p = _params(graph, xyz, density, scaling, rotation)
    cost = _edge_array(graph, cost, "cost", _F32)
    mate = _node_array(graph, mate, "mate")
    dev, P, K = graph.idx.device, graph.P, graph.K
    if P == 0:
        return p[0], p[1], p[2], p[3], torch.empty((0, 2), dtype=_I32, device=dev), dict(pairs=0, open=0, P=0)
    scratch = torch.empty((int(_lib.lib().r2_merge_scratch_bytes(P)),), dtype=torch.uint8, device=dev)
    counts = (C.c_uint * 2)()
    call("r2_merge_count", dev, P, K, graph.idx, graph.in_offsets, graph.in_edges, cost, float(max_cost), mate, p[1], p[2], scratch,
         counts)
    pairs, n_open = int(counts[0]), int(counts[1])
    Pn = P - pairs
    outs = [torch.empty((Pn, w), dtype=_F32, device=dev) for w in WIDTHS.values()]
    src = torch.empty((Pn, 2), dtype=_I32, device=dev)
    call("r2_merge_emit", dev, P, *p, scratch, Pn, *outs, src)
    return outs[0], outs[1], outs[2], outs[3], src, dict(pairs=pairs, open=n_open, P=Pn)


def merge_gaussians(xyz, density, scaling, rotation, max_cost, k=8, rounds=12, max_scale=None, graph=None):
    """All of it: the k nearest neighbours of xyz (unless a graph is given), the costs, `rounds` rounds of matching on the edges
    with cost <= max_cost, the merged cloud.  max_cost is capped at the largest finite float32: an edge whose cost is +inf
    (unusable parameters, a trace beyond max_scale^2) is never merged here, whereas match_edges with max_cost = +inf takes its
    costs literally.  -> merge_pairs' tuple."""
    require_gpu(xyz, "xyz")
    max_cost = min(float(max_cost), float(np.finfo(np.float32).max))
    if graph is None:
        graph = knn_graph(xyz, k)
    cost = merge_costs(graph, xyz, density, scaling, rotation, max_scale=max_scale)
    mate = match_edges(graph, cost, max_cost, rounds=rounds)
    return merge_pairs(graph, cost, max_cost, mate, xyz, density, scaling, rotation)


__all__ = ["merge_costs", "match_edges", "merge_pairs", "merge_gaussians", "max_trace_of"]
