"""CPU: the references of tests/graph_ref.py against hand-computed examples (a tie broken by index, a duplicate point, short
rows, invalid targets), and the new C ABI: header, ctypes binding, constants and the Python module agree."""
import os
import re

import numpy as np

from tests import graph_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# point 3 duplicates point 0; 1 and 2 are equally far from 0, 3, 4 and 5
SIX = np.array([[0, 0, 0], [1, 0, 0], [-1, 0, 0], [0, 0, 0], [0, 3, 0], [0, 0, 5]], dtype=np.float32)
SIX_IDX = np.array([[3, 1, 2], [0, 3, 2], [0, 3, 1], [0, 1, 2], [0, 3, 1], [0, 3, 1]], dtype=np.int32)
SIX_D2 = np.array([[0, 1, 1], [1, 1, 4], [1, 1, 4], [0, 1, 1], [9, 9, 10], [25, 25, 26]], dtype=np.float32)


def test_reference_knn_on_six_points():
    idx, d2 = R.knn_graph(SIX, 3)
    assert idx.dtype == np.int32 and d2.dtype == np.float32
    assert np.array_equal(idx, SIX_IDX) and np.array_equal(d2, SIX_D2)
    # the result does not depend on how the queries are chunked
    idx1, d21 = R.knn_graph(SIX, 3, chunk=1)
    assert np.array_equal(idx1, idx) and np.array_equal(d21, d2)
    # K = 1: the duplicate is the nearest of 0 and of 3; the tie 0 / 3 seen from the others goes to index 0
    idx, d2 = R.knn_graph(SIX, 1)
    assert idx[:, 0].tolist() == [3, 0, 0, 0, 0, 0] and d2[:, 0].tolist() == [0, 1, 1, 0, 9, 25]


def test_reference_knn_short_rows():
    idx, d2 = R.knn_graph(SIX, 7)
    assert np.array_equal(idx[:, 5:], np.full((6, 2), -1)) and np.all(np.isposinf(d2[:, 5:]))
    assert idx[0, :5].tolist() == [3, 1, 2, 4, 5] and d2[0, :5].tolist() == [0, 1, 1, 9, 25]
    for P in (0, 1):
        idx, d2 = R.knn_graph(SIX[:P], 3)
        assert idx.shape == (P, 3) and np.all(idx == -1) and np.all(np.isposinf(d2))


def test_reference_transpose():
    off, edges = R.transpose(SIX_IDX)
    assert off.tolist() == [0, 5, 10, 13, 18, 18, 18]
    assert edges.tolist() == [3, 6, 9, 12, 15, 1, 8, 10, 14, 17, 2, 5, 11, 0, 4, 7, 13, 16]
    # -1 and out-of-range targets are no edges
    off, edges = R.transpose(np.array([[1, -1], [7, 0], [0, 1]], dtype=np.int32))
    assert off.tolist() == [0, 2, 4, 4] and edges.tolist() == [3, 4, 0, 5]
    off, edges = R.transpose(np.zeros((0, 4), dtype=np.int32))
    assert off.tolist() == [0] and edges.size == 0


def test_reference_loss_by_hand():
    idx = np.array([[1, 2], [0, -1], [-1, -1]], dtype=np.int32)
    v = np.array([1.0, 3.0, 0.0])
    r = R.loss_and_grad(v, idx, None, 0, None, 0.5)
    assert r["loss"] == 2.5 and r["abs_sum"] == 5.0 and r["grad"].tolist() == [-0.5, 1.0, -0.5]
    assert r["indegree"].tolist() == [1, 1, 1] and r["outdegree"].tolist() == [2, 1, 0] and r["abs_terms"].tolist() == [3, 2, 1]
    r = R.loss_and_grad(v, idx, None, 1, None, 0.5)
    assert r["loss"] == 4.5 and r["grad"].tolist() == [-3.0, 4.0, -1.0]
    r = R.loss_and_grad(v, idx, None, 2, 1.5, 0.5)
    assert r["loss"] == 2.125 and r["grad"].tolist() == [0.5 * (-1.5 + 1 - 1.5), 0.5 * (1.5 + 1.5), -0.5]
    w = np.array([[2.0, 0.0], [1.0, 5.0], [5.0, 5.0]])
    r = R.loss_and_grad(v, idx, w, 0, None, 1.0, g=3.0)
    assert r["loss"] == 6.0 and r["grad"].tolist() == [3.0 * (-2 - 1), 3.0 * (1 + 2), 0.0]
    # tied values: no gradient for kind 0
    r = R.loss_and_grad(np.array([2.0, 2.0, 2.0]), idx, None, 0, None, 1.0)
    assert r["loss"] == 0.0 and r["grad"].tolist() == [0.0, 0.0, 0.0]


NEW_SYMBOLS = ("r2_knn_graph_workspace_bytes", "r2_knn_graph", "r2_graph_transpose_workspace_bytes", "r2_graph_transpose",
               "r2_graph_loss_scratch_floats", "r2_graph_loss", "r2_graph_loss_backward")


def test_header_binding_and_module_agree():
    from r2_gaussian_amd import _lib
    from r2_gaussian_amd import graph as G
    src = open(os.path.join(ROOT, "include", "r2hip.h")).read()
    for s in NEW_SYMBOLS:
        assert re.search(r"R2_API\s+(int|size_t)\s+%s\s*\(" % s, src), s
        assert s in _lib.exported_symbols()
    for name in ("R2_KNN_GRAPH_MAX_K", "R2_GRAPH_KIND_L1", "R2_GRAPH_KIND_L2", "R2_GRAPH_KIND_HUBER", "R2_GRAPH_LOSS_CHAIN",
                 "R2_GRAPH_LOSS_HUB"):
        m = re.search(r"^#define\s+%s\s+(-?\d+)\s*$" % name, src, flags=re.M)
        assert m and int(m.group(1)) == getattr(_lib, name), name
    L = _lib.lib()   # argtypes on every symbol; raises on a missing one
    assert L.r2_graph_loss_scratch_floats(0, 3) == 1 and L.r2_graph_loss_scratch_floats(2049, 1) == 2
    assert L.r2_knn_graph_workspace_bytes(0, 3) == 0
    assert L.r2_knn_graph_workspace_bytes(5000, 16) == L.r2_knn_workspace_bytes(5000)
    assert G.KINDS == {"l1": 0, "l2": 1, "huber": 2}
    for name in ("knn_graph", "graph_from_indices", "edge_weights", "graph_smoothness", "NeighbourGraph"):
        assert hasattr(G, name)
    # 8 terms per thread, 6 butterfly steps, 2 levels over the 4 waves, 1 rounding of the double total
    assert _lib.R2_GRAPH_LOSS_CHAIN == 8 + 6 + 2 + 1


def test_trainer_flags_default_off():
    from r2_gaussian_amd import train as TR
    a = TR.build_parser().parse_args(["-s", "x"])
    assert a.lambda_graph == 0.0 and a.graph_k == 8 and a.graph_every == 100
    a = TR.build_parser().parse_args(["-s", "x", "--lambda_graph", "0.01", "--graph_k", "4", "--graph_every", "50"])
    assert a.lambda_graph == 0.01 and a.graph_k == 4 and a.graph_every == 50
