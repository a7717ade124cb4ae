"""Restatement of r2_tv_prox (include/r2hip.h) and of recon.fista_tv.  Host only; the product never imports this file.

``tv_prox`` is written once and run in two precisions.  In float32 every line is one separately rounded IEEE operation in
the order the header states (NumPy float32 arithmetic rounds each add, multiply, divide and square root once and never
fuses), so it is the kernel operation for operation; in float64 the same lines are the reference the float32 error is
measured against.  The momentum factors are computed in double and rounded to the working precision, as the library does.
``fista_tv`` is the float64 loop of recon.fista_tv on a dense matrix.
"""
import numpy as np


def _shift_lower(d, ax):
    """out(v) = d(v - e_ax) where v_ax > 0, else 0."""
    out = np.zeros_like(d)
    hi = [slice(None)] * 3
    lo = [slice(None)] * 3
    hi[ax] = slice(1, None)
    lo[ax] = slice(None, -1)
    out[tuple(hi)] = d[tuple(lo)]
    return out


def _own_masked(d, ax):
    """d(v) where v_ax < n_ax - 1, else 0."""
    out = d.copy()
    last = [slice(None)] * 3
    last[ax] = slice(-1, None)
    out[tuple(last)] = 0
    return out


def div_t(d):
    """(D^T d)(v) in the header's order: t_a = lower - own, (t_x + t_y) + t_z."""
    t = [_shift_lower(d[a], a) - _own_masked(d[a], a) for a in range(3)]
    return (t[0] + t[1]) + t[2]


def diffs(x):
    """Forward differences, zero at the last index of each axis."""
    out = []
    for ax in range(3):
        d = np.zeros_like(x)
        hi = [slice(None)] * 3
        lo = [slice(None)] * 3
        hi[ax] = slice(1, None)
        lo[ax] = slice(None, -1)
        d[tuple(lo)] = x[tuple(hi)] - x[tuple(lo)]
        out.append(d)
    return out


def momenta(n_iter):
    """(t_k - 1) / t_{k+1} for k = 1 .. n_iter, in double."""
    t, out = 1.0, []
    for _ in range(n_iter):
        t_next = 0.5 * (1.0 + np.sqrt(1.0 + 4.0 * t * t))
        out.append((t - 1.0) / t_next)
        t = t_next
    return out


def tv_prox(y, lam, n_iter, lo=None, hi=None, dtype=np.float64):
    f = np.dtype(dtype).type
    y = np.asarray(y, dtype=f)
    lam = f(lam)
    lo = f(-np.inf if lo is None else lo)
    hi = f(np.inf if hi is None else hi)

    def clamp(u):
        return np.where(u < lo, lo, np.where(u > hi, hi, u)).astype(f)

    with np.errstate(all="ignore"):
        tau = f(1) / (f(12) * lam)
    if not (lam > 0 and tau > 0 and np.isfinite(tau)) or n_iter == 0:
        return clamp(y)
    r = [np.zeros_like(y) for _ in range(3)]
    p_prev = [np.zeros_like(y) for _ in range(3)]
    p = p_prev
    for mom in momenta(n_iter):
        mom = f(mom)
        x = clamp(y - lam * div_t(r))
        d = diffs(x)
        q = [r[a] + tau * d[a] for a in range(3)]
        n = np.sqrt((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2])
        m = np.where(n > f(1), n, f(1)).astype(f)
        p = [q[a] / m for a in range(3)]
        r = [p[a] + mom * (p[a] - p_prev[a]) for a in range(3)]
        p_prev = p
    out = clamp(y - lam * div_t(p))
    assert out.dtype == f
    return out


def tv_prox64(y, lam, n_iter, lo=None, hi=None):
    return tv_prox(y, lam, n_iter, lo, hi, np.float64)


def tv_prox32(y, lam, n_iter, lo=None, hi=None):
    return tv_prox(y, lam, n_iter, lo, hi, np.float32)


def tv_value(x):
    """The isotropic, unsmoothed TV (float64)."""
    d = diffs(np.asarray(x, np.float64))
    return float(np.sqrt(d[0] ** 2 + d[1] ** 2 + d[2] ** 2).sum())


def objective(x, y, lam):
    """F(x) = 1/2 |x - y|^2 + lam TV(x) (float64)."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    return 0.5 * float(((x - y) ** 2).sum()) + float(lam) * tv_value(x)


def operator_norm_bound(A):
    """max(A 1) max(A^T 1) = |A|_inf |A|_1 for a matrix without negative entries."""
    return float((A @ np.ones(A.shape[1])).max() * (A.T @ np.ones(A.shape[0])).max())


def fista_tv(A, b, shape, niter, lam_rel, tviter, L=None, x0=None, nonneg=True):
    """recon.fista_tv in float64 on a dense A -> (the iterates x_1 .. x_niter, the absolute lambda, L)."""
    A = np.asarray(A, np.float64)
    b = np.asarray(b, np.float64)
    lam = lam_rel * np.abs(A.T @ b).max()
    L = operator_norm_bound(A) if L is None else float(L)
    x = np.zeros(A.shape[1]) if x0 is None else np.asarray(x0, np.float64).ravel().copy()
    y, t, out = x.copy(), 1.0, []
    for _ in range(niter):
        z = y - (A.T @ (A @ y - b)) / L
        x_new = tv_prox64(z.reshape(shape), lam / L, tviter, 0.0 if nonneg else None).ravel()
        t_next = 0.5 * (1.0 + np.sqrt(1.0 + 4.0 * t * t))
        y = x_new + ((t - 1.0) / t_next) * (x_new - x)
        x, t = x_new, t_next
        out.append(x.copy())
    return out, lam, L


def fista_objective(A, b, x, lam, shape):
    x = np.asarray(x, np.float64).ravel()
    return 0.5 * float(((A @ x - b) ** 2).sum()) + lam * tv_value(x.reshape(shape))
