"""Float64 restatement of the iterative reconstructions (r2_gaussian_amd/recon.py) on a dense system matrix, and of the TV
discretisation of r2_tv_descent (include/r2hip.h).  Host only; the product never imports this file.

``dense_A`` builds A column by column by projecting one-hot volumes through the projector's own float64 restatement
(tests/projector_ref.py) on the float32 rays the kernel is given.  That restatement cannot take the kernel's float32
decisions for rays whose sample count or hit/miss sits on a boundary, so ``dense_A`` reports those rays and the tests choose
geometries without any.
"""
import numpy as np

from r2_gaussian_amd import projector as K
from r2_gaussian_amd import scene as S
from tests import projector_ref as PR

EPS = 1e-8


def scene_geometry(cfg, angles):
    """The views and the scene-unit volume extent / centre ``projector.project`` uses for a raw config; and its scale."""
    scale = 2.0 / max(cfg["sVoxel"])
    H, W = (int(n) for n in cfg["nDetector"])
    views = [S.make_view(float(a), (H, W), cfg) for a in np.asarray(angles, np.float64).reshape(-1)]
    return views, [s * scale for s in cfg["sVoxel"]], [o * scale for o in cfg["offOrigin"]], scale


def dense_A(views, sVoxel, center, nVoxel, accuracy):
    """-> (A [V*H*W, nx*ny*nz] float64 in scene units, boundary: bool [V*H*W] rays on an n or hit/miss boundary)."""
    nVoxel = tuple(int(n) for n in nVoxel)
    cone = views[0].mode == 1
    H, W = views[0].image_height, views[0].image_width
    rays32 = K.ray_params(views, sVoxel, center, nVoxel)
    dvox = np.asarray(sVoxel, np.float64) / np.asarray(nVoxel)
    N = int(np.prod(nVoxel))
    A = np.zeros((len(views) * H * W, N))
    boundary = None
    for v in range(N):
        e = np.zeros(N)
        e[v] = 1.0
        r = PR.project(e.reshape(nVoxel), rays32, cone, dvox, accuracy, H, W)
        A[:, v] = r["value"]
        if boundary is None:
            boundary = (r["n_lo"] != r["n_hi"]) | r["hitmiss"]
    return A, boundary


def dense_A_cfg(cfg, angles, accuracy=None):
    """A of ``projector.project`` for a raw config (A_scene / scale), and the boundary rays."""
    views, sV, ctr, scale = scene_geometry(cfg, angles)
    acc = cfg.get("accuracy", 0.5) if accuracy is None else accuracy
    A, bd = dense_A(views, sV, ctr, cfg["nVoxel"], acc)
    return A / scale, bd


def cgls(A, b, niter):
    """-> list of the iterates x_1..x_niter and the residual norms, x0 = 0."""
    x = np.zeros(A.shape[1])
    r = b.copy()
    p = A.T @ r
    gamma = p @ p
    xs, l2 = [], []
    for _ in range(niter):
        q = A @ p
        qq = q @ q
        alpha = gamma / qq if qq > 0 else 0.0
        x = x + alpha * p
        r = r - alpha * q
        s = A.T @ r
        gn = s @ s
        beta = gn / gamma if gamma > 0 else 0.0
        p = s + beta * p
        gamma = gn
        xs.append(x.copy())
        l2.append(np.linalg.norm(r))
    return xs, l2


def _inv0(a):
    out = np.zeros_like(a)
    out[a > 0] = 1.0 / a[a > 0]
    return out


def sart_weights(A, rows_per_view, blocksize):
    V = A.shape[0] // rows_per_view
    blocks = [(v0, min(v0 + blocksize, V)) for v0 in range(0, V, blocksize)]
    Wt = _inv0(A @ np.ones(A.shape[1]))
    Vinv = [_inv0(A[v0 * rows_per_view:v1 * rows_per_view].T @ np.ones((v1 - v0) * rows_per_view)) for v0, v1 in blocks]
    return blocks, Wt, Vinv


def sart_sweep(A, b, x, lam, rows_per_view, blocks, Wt, Vinv, nonneg=True):
    for (v0, v1), vi in zip(blocks, Vinv):
        sl = slice(v0 * rows_per_view, v1 * rows_per_view)
        x = x + lam * vi * (A[sl].T @ (Wt[sl] * (b[sl] - A[sl] @ x)))
        if nonneg:
            x = np.maximum(x, 0.0)
    return x


def ossart(A, b, rows_per_view, niter, blocksize, lmbda=1.0, lmbda_red=0.999, nonneg=True, x0=None):
    """-> list of the iterates after each sweep."""
    blocks, Wt, Vinv = sart_weights(A, rows_per_view, blocksize)
    x = np.zeros(A.shape[1]) if x0 is None else x0.astype(np.float64).copy()
    lam = lmbda
    out = []
    for _ in range(niter):
        x = sart_sweep(A, b, x, lam, rows_per_view, blocks, Wt, Vinv, nonneg)
        lam *= lmbda_red
        out.append(x.copy())
    return out


def tv_value(x, eps=EPS):
    d = _diffs(x)
    return float(np.sqrt(d[0] ** 2 + d[1] ** 2 + d[2] ** 2 + eps).sum())


def _diffs(x):
    out = []
    for ax in range(3):
        d = np.zeros_like(x)
        sl_hi = [slice(None)] * 3
        sl_lo = [slice(None)] * 3
        sl_hi[ax] = slice(1, None)
        sl_lo[ax] = slice(None, -1)
        d[tuple(sl_lo)] = x[tuple(sl_hi)] - x[tuple(sl_lo)]
        out.append(d)
    return out


def tv_grad(x, eps=EPS):
    """grad TV_eps of a 3-D array (forward differences, zero past the last index)."""
    x = np.asarray(x, np.float64)
    dx, dy, dz = _diffs(x)
    s = np.sqrt(dx ** 2 + dy ** 2 + dz ** 2 + eps)
    g = -(dx + dy + dz) / s
    for ax, d in enumerate((dx, dy, dz)):
        t = d / s
        sl_hi = [slice(None)] * 3
        sl_lo = [slice(None)] * 3
        sl_hi[ax] = slice(1, None)
        sl_lo[ax] = slice(None, -1)
        g[tuple(sl_hi)] += t[tuple(sl_lo)]
    return g


def tv_descent(x, step, n_iter, eps=EPS):
    x = np.asarray(x, np.float64).copy()
    for _ in range(n_iter):
        g = tv_grad(x, eps)
        n = np.linalg.norm(g)
        if n > 0:
            x = x - step * g / n
    return x


def os_asd_pocs(A, b, shape, rows_per_view, niter, blocksize, tviter=20, maxl2err=0.0, alpha=0.002, lmbda=1.0,
                lmbda_red=0.9999, alpha_red=0.95, rmax=0.94, decisions=None):
    """Sidky & Pan's loop as recon.os_asd_pocs states it.  ``decisions``: optional list of booleans (the dtvg reductions
    to take, e.g. the kernel's), so that a run can be followed through decisions that sit on a float boundary.
    -> (x, trace with per-iteration x_sart, dd, dp, dg, dtvg, reduced, c, stopped)."""
    blocks, Wt, Vinv = sart_weights(A, rows_per_view, blocksize)
    x = np.zeros(A.shape[1])
    lam = lmbda
    dtvg = 0.0
    trace = {k: [] for k in ("x_sart", "dd", "dp", "dg", "dtvg", "reduced", "c", "x")}
    for it in range(niter):
        x_prev = x.copy()
        x = sart_sweep(A, b, x, lam, rows_per_view, blocks, Wt, Vinv, True)
        x_sart = x.copy()
        dd = np.linalg.norm(A @ x_sart - b)
        dp = np.linalg.norm(x_sart - x_prev)
        if it == 0:
            dtvg = alpha * dp
        x = tv_descent(x.reshape(shape), dtvg, tviter).reshape(-1)
        dg = np.linalg.norm(x - x_sart)
        reduced = bool(dg > rmax * dp and dd > maxl2err) if decisions is None else bool(decisions[it])
        if reduced:
            dtvg *= alpha_red
        lam *= lmbda_red
        c = float((x - x_sart) @ (x_sart - x_prev)) / max(dg * dp, 1e-6)
        for k, v in (("x_sart", x_sart), ("dd", dd), ("dp", dp), ("dg", dg), ("dtvg", dtvg), ("reduced", reduced), ("c", c),
                     ("x", x.copy())):
            trace[k].append(v)
        if c < -0.99 and dd <= maxl2err:
            break
    return x, trace
