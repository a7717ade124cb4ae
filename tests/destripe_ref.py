"""Restatement of the stripe-removal entries (include/r2hip.h: r2_proj_destripe_sort, r2_proj_destripe_mean) in NumPy / SciPy.
Host only; the product never imports this file.

The sort method is NumPy's stable argsort, SciPy's median filter and ``put_along_axis``: none of them shares anything with the
kernels' key sort and selection network.  The mean method is the header's operations one by one: the sum over the views in
float64 in the views' order, then float32 operations that NumPy rounds once each.  tests/test_destripe_cpu.py pins both to
facts that share nothing with them.
"""
import numpy as np
import scipy.ndimage as ndimage

F32 = np.float32


def _stack(src):
    x = np.asarray(src, dtype=F32)
    return (x[None] if x.ndim == 2 else x), x.ndim == 2


def destripe_sort(src, k):
    """r2_proj_destripe_sort for src [V,H,W] (or [H,W], one view) -> float32 of src's shape."""
    x, single = _stack(src)
    x = np.where(np.isnan(x), F32(np.inf), x)
    order = np.argsort(x, axis=0, kind="stable")                                 # I(r, h, w)
    S = np.take_along_axis(x, order, axis=0)
    M = ndimage.median_filter(S, size=(1, 1, k), mode="nearest")
    out = np.empty_like(x)
    np.put_along_axis(out, order, M, axis=0)
    return out[0] if single else out


def destripe_mean(src, k):
    """r2_proj_destripe_mean for src [V,H,W] (or [H,W]) -> (dst, offsets [H,W]), float32."""
    x, single = _stack(src)
    V = x.shape[0]
    acc = np.zeros(x.shape[1:], dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for v in range(V):
            acc = acc + x[v].astype(np.float64)
        m = (acc / V).astype(F32)
        window = np.where(np.isnan(m), F32(np.inf), m)
        s = ndimage.median_filter(window, size=(1, k), mode="nearest")
        d = m - s
        dst = x - d[None]
    assert d.dtype == F32 and dst.dtype == F32
    return (dst[0] if single else dst), d


# ---- the cases the CPU and the GPU tests share ---------------------------------------------------------------------------------

def case_stack(V, H, W, seed=0):
    """Smooth along the columns plus noise, every value distinct within its pixel's column with near certainty; float32."""
    rng = np.random.RandomState(5000 + seed + 3 * V + 7 * H + 13 * W)
    base = np.sin(np.arange(W) * 0.21)[None, None, :] * np.cos(np.arange(V) * 0.05)[:, None, None]
    return (base + rng.randn(V, H, W) * 0.1).astype(F32)


def ellipse_sinogram(V=360, H=2, W=256):
    """An analytic parallel-beam sinogram [V,H,W] (float64) of four ellipses, the same in every detector row up to a scale:
    an ellipse of density rho, half axes a, b, centre (x0, y0) and rotation phi has the line integral
    2 rho a b sqrt(s2 - (t - t0)^2) / s2 with s2 = a^2 cos^2(theta - phi) + b^2 sin^2(theta - phi), t0 = x0 cos theta + y0 sin theta."""
    theta = np.arange(V)[:, None] * (2.0 * np.pi / V)
    t = (np.arange(W)[None, :] - (W - 1) / 2.0) / (W / 2.0)
    sino = np.zeros((V, W))
    for rho, a, b, x0, y0, phi in ((1.0, 0.69, 0.92, 0.0, 0.0, 0.0), (-0.6, 0.55, 0.75, 0.0, -0.02, 0.0),
                                   (0.4, 0.11, 0.31, 0.22, 0.0, -0.3), (0.5, 0.16, 0.21, -0.25, 0.3, 0.9)):
        s2 = a * a * np.cos(theta - phi) ** 2 + b * b * np.sin(theta - phi) ** 2
        t0 = x0 * np.cos(theta) + y0 * np.sin(theta)
        sino += 2.0 * rho * a * b * np.sqrt(np.maximum(s2 - (t - t0) ** 2, 0.0)) / s2
    return np.stack([sino * (1.0 - 0.1 * h) for h in range(H)], axis=1)
