"""CPU references of the neighbour-graph operators (include/r2hip.h: r2_knn_graph, r2_graph_transpose, r2_graph_loss):
a brute-force k-NN in float32 with the contract's operation order, the transpose by a stable argsort, and the loss with its
gradient in float64 together with the sums of absolute terms that the tests' error bounds are made of."""
import numpy as np


def knn_graph(points, K, chunk=512):
    """-> idx [P, K] int32, dist2 [P, K] float32: per row the first K of all j != i in (dist2 ascending, j ascending) order,
    dist2 = ((dx*dx + dy*dy) + dz*dz) in float32 with d = other - self; missing slots (P - 1 < K) are -1 / +inf."""
    pts = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
    P = pts.shape[0]
    idx = np.full((P, K), -1, dtype=np.int32)
    dist2 = np.full((P, K), np.inf, dtype=np.float32)
    n = min(K, max(P - 1, 0))
    if n == 0:
        return idx, dist2
    cols = np.arange(P, dtype=np.int64)
    for a in range(0, P, chunk):
        q = pts[a:a + chunk]
        dx = pts[None, :, 0] - q[:, None, 0]
        dy = pts[None, :, 1] - q[:, None, 1]
        dz = pts[None, :, 2] - q[:, None, 2]
        d = (dx * dx + dy * dy) + dz * dz
        assert d.dtype == np.float32
        # the n + 1 smallest of a row (self included) are all <= its value at sorted position n: only those need the full sort
        thr = np.partition(d, n, axis=1)[:, n]
        for r in range(q.shape[0]):
            i = a + r
            jj = cols[d[r] <= thr[r]]
            jj = jj[jj != i]   # self excluded by index
            dj = d[r][jj]
            order = np.lexsort((jj, dj))[:n]   # primary key dist2, ties by index
            idx[i, :n] = jj[order]
            dist2[i, :n] = dj[order]
    return idx, dist2


def transpose(idx):
    """-> in_offsets [P + 1] int32, in_edges [E] int32: the valid edges (target in [0, P)) grouped by target, ascending edge id
    inside a group (stable sort)."""
    idx = np.asarray(idx)
    P = idx.shape[0]
    flat = idx.reshape(-1).astype(np.int64)
    valid = (flat >= 0) & (flat < P)
    key = np.where(valid, flat, P)
    order = np.argsort(key, kind="stable")
    E = int(valid.sum())
    counts = np.bincount(key[valid], minlength=P)[:P] if P else np.zeros(0, dtype=np.int64)
    in_offsets = np.zeros(P + 1, dtype=np.int32)
    in_offsets[1:] = np.cumsum(counts)
    return in_offsets, order[:E].astype(np.int32)


def _phi(x, kind, delta):
    if kind == 0:
        return np.abs(x), np.sign(x)
    if kind == 1:
        return x * x, 2.0 * x
    ax = np.abs(x)
    return np.where(ax <= delta, 0.5 * x * x, delta * (ax - 0.5 * delta)), np.where(ax <= delta, x, delta * np.sign(x))


def loss_and_grad(v, idx, w, kind, delta, scale, g=1.0):
    """float64: -> dict(loss, abs_sum = sum |w phi| (unscaled), grad [P], abs_terms [P] = per node the sum of |w phi'| over its
    own and its incoming edges (unscaled), indegree [P], outdegree [P])."""
    v = np.asarray(v, dtype=np.float64).reshape(-1)
    idx = np.asarray(idx)
    P, K = idx.shape
    valid = (idx >= 0) & (idx < P)
    j = np.where(valid, idx, 0).astype(np.int64)
    ww = np.ones((P, K)) if w is None else np.asarray(w, dtype=np.float64)
    x = v[:, None] - v[j] if P else np.zeros((0, K))
    phi, dphi = _phi(x, kind, float(delta) if delta else 0.0)
    t = np.where(valid, ww * phi, 0.0)
    dt = np.where(valid, ww * dphi, 0.0)
    grad = dt.sum(1)
    np.subtract.at(grad, j[valid], dt[valid])
    abs_terms = np.abs(dt).sum(1)
    np.add.at(abs_terms, j[valid], np.abs(dt[valid]))
    indeg = np.bincount(j[valid], minlength=P)[:P] if P else np.zeros(0, dtype=np.int64)
    return dict(loss=float(scale) * t.sum(), abs_sum=np.abs(t).sum(), grad=float(g) * float(scale) * grad, abs_terms=abs_terms,
                indegree=indeg, outdegree=valid.sum(1))
