"""Float64 restatement of the training losses (r2_gaussian/utils/loss_utils.py:19-104) and the derived float32 error bounds
the fused kernels (csrc/loss_ops.hip) are checked against.  Host only: the SSIM blurs are separable numpy sums, never a
convolution on the GPU (the vendor convolution can fault this stack, see loss_ops.hip).

Bounds follow from float32 rounding, in the style of oracle/parity.py: u = 2^-24 is the unit roundoff, a float sum or
product chain of n roundings is accurate to n u times the sum of the magnitudes of its terms (gamma_n ~ n u), and errors of
inputs propagate to first order through the exact derivatives of each expression.  The rounding counts follow the kernels:

* a moment m = W*x (or W*x^2, W*xy) is an 11-tap horizontal then an 11-tap vertical sequential sum, each tap a product with
  the window rounded to float once: 2 x (11 + 11) + 2 + 1 (the square) < N_BLUR = 48 roundings, relative to W*|terms|;
* the SSIM algebra after the moments (s = e - m^2, A1, A2, B1, B2, 1 / (B1 B2), S, D1..D3) is a few roundings per
  quantity; N_OP = 8 per step bounds each, and the float constants C1, C2 are themselves u-relative;
* dL/dx(p) blurs D1..D3 the same way (N_BLUR) and combines them with x, y and 1 / N (N_OP);
* the per-block sums are a 64-lane butterfly (6 levels) and a 4-wave sequential sum (3): 9 roundings; the fold of the
  per-block sums is in double (error ~ 2^-53 per term) and the result is rounded to float once.

The conditioning term is what the float cancellation in s = e - m^2 costs: delta s ~ N_BLUR u (e + m^2), propagated through
S and D1..D3.  It dominates in smooth bright regions, where the reference's own float32 evaluation has the same error.
"""
import math

import numpy as np

U = 2.0 ** -24          # float32 unit roundoff
U64 = 2.0 ** -53
N_BLUR = 48
N_OP = 8
N_BLOCK = 9             # per-block tree sum: 6 butterfly levels + 3 sequential wave sums
C1, C2 = 0.01 ** 2, 0.03 ** 2
LT = 16                 # the kernels' output tile


def window64(size=11, sigma=1.5):
    g = np.array([math.exp(-((i - size // 2) ** 2) / (2.0 * sigma ** 2)) for i in range(size)], np.float64)
    return g / g.sum()


def blur64(a, w=None):
    """Zero-padded separable 11 x 11 Gaussian correlation (= convolution: the window is symmetric) of a 2D array in float64."""
    w = window64() if w is None else w
    h = len(w) // 2
    H, W = a.shape
    p = np.zeros((H, W + 2 * h))
    p[:, h:h + W] = a
    r = sum(w[k] * p[:, k:k + W] for k in range(len(w)))
    p = np.zeros((H + 2 * h, W))
    p[h:h + H] = r
    return sum(w[k] * p[k:k + H] for k in range(len(w)))


def l1_ssim64(img, gt, w_l1=1.0, w_ssim=0.25):
    """-> dict: loss = w_l1 mean|x - y| + w_ssim (1 - mean S), its parts l1, ssim, dL/dimg as `grad`, and the per-pixel maps
    S, m1, m2, e11, e22, e12, A1, A2, B1, B2, D1, D2, D3 (all float64)."""
    x = np.asarray(img, np.float64).reshape(np.shape(img)[-2:])
    y = np.asarray(gt, np.float64).reshape(np.shape(gt)[-2:])
    assert x.shape == y.shape
    N = x.size
    m1, m2, e11, e22, e12 = blur64(x), blur64(y), blur64(x * x), blur64(y * y), blur64(x * y)
    s1, s2, s12 = e11 - m1 * m1, e22 - m2 * m2, e12 - m1 * m2
    A1, A2 = 2 * m1 * m2 + C1, 2 * s12 + C2
    B1, B2 = m1 * m1 + m2 * m2 + C1, s1 + s2 + C2
    inv = 1.0 / (B1 * B2)
    S = A1 * A2 * inv
    D1 = 2 * m2 * (A2 - A1) * inv - S * (2 * m1 / B1 - 2 * m1 / B2)   # dS/dm1, with s1 and s12 depending on m1
    D2 = -S / B2                                                       # dS/d(W*x^2)
    D3 = 2 * A1 * inv                                                  # dS/d(W*xy)
    l1, ssim = np.abs(x - y).mean(), S.mean()
    grad = w_l1 * np.sign(x - y) / N - w_ssim / N * (blur64(D1) + 2 * x * blur64(D2) + y * blur64(D3))
    return dict(loss=w_l1 * l1 + w_ssim * (1.0 - ssim), l1=l1, ssim=ssim, grad=grad, S=S, m1=m1, m2=m2, e11=e11, e22=e22,
                e12=e12, A1=A1, A2=A2, B1=B1, B2=B2, D1=D1, D2=D2, D3=D3, x=x, y=y, w_l1=w_l1, w_ssim=w_ssim)


def n_blocks(H, W):
    return ((H + LT - 1) // LT) * ((W + LT - 1) // LT)


def l1_ssim_bounds(r):
    """-> dict of derived float32 error bounds for a result `r` of l1_ssim64 on non-negative images: `grad` (per pixel),
    `l1`, `ssim`, `loss` (scalars), `ssim_float_fold` (the scalar bound had the per-block sums been folded in float), and
    `cond_ok` (first-order propagation is valid: the B2 error stays below half of B2 everywhere)."""
    x, y = r["x"], r["y"]
    assert (x >= 0).all() and (y >= 0).all(), "the bounds are derived for non-negative images (projections)"
    m1, m2, e11, e22, e12 = r["m1"], r["m2"], r["e11"], r["e22"], r["e12"]
    A1, A2, B1, B2, S = r["A1"], r["A2"], r["B1"], r["B2"], r["S"]
    N = x.size
    k = N_BLUR * U
    # absolute errors of the moments: relative to W*|terms| (= the moment itself for non-negative x, y)
    dm1, dm2 = k * m1, k * m2
    # A1, B1, A2, B2 from the moments, plus their own rounding and the float constants' (C1, C2 relative u)
    dA1 = 2 * (m1 * dm2 + m2 * dm1) + N_OP * U * A1
    dB1 = 2 * (m1 * dm1 + m2 * dm2) + N_OP * U * B1
    dA2 = 2 * (k * e12 + m1 * dm2 + m2 * dm1) + N_OP * U * (2 * e12 + 2 * m1 * m2 + C2)
    dB2 = k * (e11 + e22) + 2 * (m1 * dm1 + m2 * dm2) + N_OP * U * (e11 + e22 + m1 * m1 + m2 * m2 + C2)
    cond_ok = bool((dB2 < 0.5 * B2).all())
    rA1, rB1, rB2 = dA1 / A1, dB1 / B1, dB2 / B2
    inv = 1.0 / (B1 * B2)
    rinv = rB1 + rB2 + N_OP * U
    dS = np.abs(A1 * A2) * inv * (rA1 + rinv + N_OP * U) + A1 * inv * dA2
    # D1 = a - b, a = 2 m2 (A2 - A1) inv, b = S 2 m1 (1/B1 - 1/B2)
    a = 2 * m2 * (A2 - A1) * inv
    da = 2 * inv * (dm2 * np.abs(A2 - A1) + m2 * (dA2 + dA1)) + np.abs(a) * (rinv + N_OP * U)
    q = 1.0 / B1 - 1.0 / B2
    dq = rB1 / B1 + rB2 / B2 + N_OP * U * (1.0 / B1 + 1.0 / B2)
    b = S * 2 * m1 * q
    db = 2 * (dS * m1 * np.abs(q) + np.abs(S) * (dm1 * np.abs(q) + m1 * dq)) + N_OP * U * np.abs(b)
    dD1 = da + db + N_OP * U * (np.abs(a) + np.abs(b))
    D2, D3 = r["D2"], r["D3"]
    dD2 = dS / B2 + np.abs(D2) * (rB2 + N_OP * U)
    dD3 = np.abs(D3) * (rA1 + rinv + N_OP * U)
    # dL/dx(p) = -w_ssim / N (W*D1 + 2 x W*D2 + y W*D3) + w_l1 sign(x - y) / N: the blurs' own rounding on W*|D| and the
    # propagated D errors, then the combination and the scaling by 1/N
    G = blur64(np.abs(r["D1"])) + 2 * x * blur64(np.abs(D2)) + y * blur64(np.abs(D3))
    dG = blur64(dD1) + 2 * x * blur64(dD2) + y * blur64(dD3)
    ws, wl = abs(r["w_ssim"]), abs(r["w_l1"])
    grad = ws / N * ((N_BLUR + N_OP) * U * G + dG) + N_OP * U * wl / N
    # scalars: per-pixel errors, the per-block float tree sums, a double fold, one rounding to float
    nb = n_blocks(*x.shape)
    sum_abs_S, sum_l1 = np.abs(S).sum(), np.abs(x - y).sum()
    fold64 = (nb + 8) * U64
    ssim = (dS.sum() + (N_BLOCK * U + fold64) * sum_abs_S) / N + U * abs(r["ssim"])
    l1 = ((1 + N_BLOCK) * U + fold64) * sum_l1 / N + U * r["l1"]
    loss = wl * l1 + ws * ssim + U * abs(r["loss"])
    # the same with the fold in float: per thread ceil(nb / 256) sequential sums, a butterfly and a 4-wave sum
    n_fold32 = -(-nb // 256) + 6 + 3 + 1
    ssim_float_fold = (dS.sum() + (N_BLOCK + n_fold32) * U * sum_abs_S) / N + U * abs(r["ssim"])
    return dict(grad=grad, ssim=ssim, l1=l1, loss=loss, ssim_float_fold=ssim_float_fold, cond_ok=cond_ok, G=G)


# ---------------------------------------------------------------------------------------------------------------- TV
def tv3d64(vol):
    """tv_3d_loss(vol, "mean") in float64 -> (tv, dtv/dvol, sum |d|, pair count).  No neighbour pairs (1 x 1 x 1): 0 / 0 = NaN
    and a zero gradient, as torch evaluates the reference (the gradient of an empty diff is zero)."""
    v = np.asarray(vol, np.float64)
    g = np.zeros_like(v)
    total = 0.0
    for ax in range(3):
        d = np.diff(v, axis=ax)
        total += np.abs(d).sum()
        s = np.sign(d)
        lo = [slice(None)] * 3
        hi = [slice(None)] * 3
        lo[ax], hi[ax] = slice(0, -1), slice(1, None)
        g[tuple(lo)] -= s
        g[tuple(hi)] += s
    n = v.shape
    cnt = (n[0] - 1) * n[1] * n[2] + n[0] * (n[1] - 1) * n[2] + n[0] * n[1] * (n[2] - 1)
    if cnt == 0:
        return math.nan, np.zeros_like(v), total, 0
    return total / cnt, g / cnt, total, cnt


def tv3d_bounds(vol, total, cnt, grad):
    """Derived float32 bounds of the fused TV: the gradient is weight * g / cnt with g an exact integer sum of exact signs (a
    float difference has the sign of the exact one), so 3 roundings of |ref|; the value sums |d| (rounded once each) in at
    most 3 per thread, the 9-rounding block tree, a double fold, one division and one rounding to float.  Also the value
    bound had the fold been in float."""
    nb = -(-int(np.prod(vol.shape)) // 256)
    if cnt == 0:
        return dict(grad=np.zeros_like(grad), tv=0.0, tv_float_fold=0.0)
    tv = ((3 + N_BLOCK) * U + (nb + 8) * U64) * total / cnt + 2 * U * total / cnt
    tv_float_fold = (3 + N_BLOCK + (-(-nb // 256) + 6 + 3 + 2)) * U * total / cnt
    return dict(grad=3 * U * np.abs(grad), tv=tv, tv_float_fold=tv_float_fold)


# ------------------------------------------------------------------------------------------ the kernels' float folds
def float_fold(parts, nthreads=256):
    """The fold the loss kernels used before their scalars moved to double: per thread a sequential float32 sum of
    parts[t::256], a 64-lane xor butterfly per wave, then the 4 wave sums in order.  Emulated on the host, bit for bit in
    IEEE float32, from the per-block partial sums a kernel left in its scratch."""
    p = np.asarray(parts, np.float32).reshape(-1)
    acc = np.zeros(nthreads, np.float32)
    for i in range(0, p.size, nthreads):
        c = p[i:i + nthreads]
        acc[:c.size] = acc[:c.size] + c
    waves = acc.reshape(-1, 64)
    lane = np.arange(64)
    for d in (32, 16, 8, 4, 2, 1):
        waves = waves + waves[:, lane ^ d]
    t = waves[0, 0]
    for w in range(1, waves.shape[0]):
        t = np.float32(t + waves[w, 0])
    return t
