"""Float64 restatement of the weighted image loss (r2_loss_l1_ssim_weighted of include/r2hip.h, csrc/loss_ops.hip) and the
derived float32 error bounds its kernels are checked against.  Host only, built on tests/loss_ref.py.

The loss: a weight counts only where it is > 0 (negative, zero and NaN weights are 0).  With w the counted weights,
y' = gt where w > 0 and the image's own value elsewhere (held constant), S the SSIM map of (x, y') and D1..D3 its partial
derivatives exactly as loss_ref.l1_ssim64 forms them,

    sum_w = sum w,  l1 = sum w |x - y'| / sum_w,  ssim = sum w S / sum_w,  loss = w_l1 l1 + w_ssim (1 - ssim),
    dL/dx(p) = w_l1 w(p) sign(x(p) - y'(p)) / sum_w - w_ssim / sum_w (W*(w D1) + 2 x W*(w D2) + y' W*(w D3))(p),

and sum_w = 0 gives l1 = 0, ssim = 1, loss = 0 and a zero gradient.

The bounds extend loss_ref.l1_ssim_bounds (same notation: u = 2^-24, N_BLUR, N_OP, N_BLOCK; its per-pixel bounds dS, dD1..dD3 of
the SSIM algebra are restated here because that function does not return them), following the weighted kernels' roundings:

* a weighted derivative map w D_i and the summands w S, w |x - y'| are one more float product each: u relative on top of the
  error of D_i, S (|x - y'| is itself one rounding);
* sum_w is summed like the other per-block sums (N_BLOCK roundings of positive terms), folded in double ((nb + 8) 2^-53) and
  rounded to float once: relative error E_SUM = (N_BLOCK + 1) u + (nb + 8) 2^-53.  The scalars divide the double folds by the
  double sum_w (no rounding to float: N_BLOCK u + the fold), the gradient is scaled by 1 / float(sum_w);
* the gradient is the unweighted expression with 1 / N -> 1 / sum_w: the blurs' own rounding on W*(w |D|), the propagated
  errors W*(w dD + u w |D|), the combination (N_OP), and E_SUM relative to the magnitude of both terms.
"""
import numpy as np

from tests import loss_ref as R

U, U64, N_BLUR, N_OP, N_BLOCK = R.U, R.U64, R.N_BLUR, R.N_OP, R.N_BLOCK


def counted(weights):
    """The weights as the loss counts them, in float64: values that are not > 0 (also NaN) are 0."""
    w = np.asarray(weights, np.float64)
    with np.errstate(invalid="ignore"):
        return np.where(w > 0, w, 0.0)


def weighted_l1_ssim64(img, gt, weights, w_l1=1.0, w_ssim=0.25):
    """-> dict: loss, l1, ssim, sum_w, grad, the counted weights `w`, the measurement used `yp`, and `r` = loss_ref.l1_ssim64 of
    (img, yp) with its per-pixel maps.  weights None = ones."""
    x = np.asarray(img, np.float64).reshape(np.shape(img)[-2:])
    y = np.asarray(gt, np.float64).reshape(np.shape(gt)[-2:])
    w = np.ones_like(x) if weights is None else counted(weights).reshape(x.shape)
    yp = np.where(w > 0, y, x)
    r = R.l1_ssim64(x, yp, w_l1, w_ssim)
    sw = w.sum()
    if sw == 0:
        return dict(loss=0.0, l1=0.0, ssim=1.0, sum_w=0.0, grad=np.zeros_like(x), w=w, yp=yp, r=r, w_l1=w_l1, w_ssim=w_ssim)
    l1 = (w * np.abs(x - yp)).sum() / sw
    ssim = (w * r["S"]).sum() / sw
    grad = w_l1 * w * np.sign(x - yp) / sw - w_ssim / sw * (R.blur64(w * r["D1"]) + 2 * x * R.blur64(w * r["D2"]) +
                                                           yp * R.blur64(w * r["D3"]))
    return dict(loss=w_l1 * l1 + w_ssim * (1.0 - ssim), l1=l1, ssim=ssim, sum_w=sw, grad=grad, w=w, yp=yp, r=r, w_l1=w_l1,
                w_ssim=w_ssim)


def _ssim_algebra_bounds(r):
    """dS, dD1, dD2, dD3 (per pixel) and cond_ok of loss_ref.l1_ssim_bounds, step for step."""
    m1, m2, e11, e22, e12 = r["m1"], r["m2"], r["e11"], r["e22"], r["e12"]
    A1, A2, B1, B2, S = r["A1"], r["A2"], r["B1"], r["B2"], r["S"]
    k = N_BLUR * U
    dm1, dm2 = k * m1, k * m2
    dA1 = 2 * (m1 * dm2 + m2 * dm1) + N_OP * U * A1
    dB1 = 2 * (m1 * dm1 + m2 * dm2) + N_OP * U * B1
    dA2 = 2 * (k * e12 + m1 * dm2 + m2 * dm1) + N_OP * U * (2 * e12 + 2 * m1 * m2 + R.C2)
    dB2 = k * (e11 + e22) + 2 * (m1 * dm1 + m2 * dm2) + N_OP * U * (e11 + e22 + m1 * m1 + m2 * m2 + R.C2)
    cond_ok = bool((dB2 < 0.5 * B2).all())
    rA1, rB1, rB2 = dA1 / A1, dB1 / B1, dB2 / B2
    inv = 1.0 / (B1 * B2)
    rinv = rB1 + rB2 + N_OP * U
    dS = np.abs(A1 * A2) * inv * (rA1 + rinv + N_OP * U) + A1 * inv * dA2
    a = 2 * m2 * (A2 - A1) * inv
    da = 2 * inv * (dm2 * np.abs(A2 - A1) + m2 * (dA2 + dA1)) + np.abs(a) * (rinv + N_OP * U)
    q = 1.0 / B1 - 1.0 / B2
    dq = rB1 / B1 + rB2 / B2 + N_OP * U * (1.0 / B1 + 1.0 / B2)
    b = S * 2 * m1 * q
    db = 2 * (dS * m1 * np.abs(q) + np.abs(S) * (dm1 * np.abs(q) + m1 * dq)) + N_OP * U * np.abs(b)
    dD1 = da + db + N_OP * U * (np.abs(a) + np.abs(b))
    dD2 = dS / B2 + np.abs(r["D2"]) * (rB2 + N_OP * U)
    dD3 = np.abs(r["D3"]) * (rA1 + rinv + N_OP * U)
    return dS, dD1, dD2, dD3, cond_ok


def weighted_bounds(ref):
    """-> dict of derived float32 error bounds for a result of weighted_l1_ssim64 on non-negative images: `grad` (per pixel),
    `l1`, `ssim`, `loss`, `sum_w` (scalars) and `cond_ok` (of (x, y'), as loss_ref.l1_ssim_bounds defines it).  sum_w = 0: the
    kernels' values are exact (every bound is 0)."""
    r, w = ref["r"], ref["w"]
    x, yp = r["x"], r["y"]
    assert (x >= 0).all() and (yp >= 0).all(), "the bounds are derived for non-negative images (projections)"
    assert np.isfinite(w).all()
    dS, dD1, dD2, dD3, cond_ok = _ssim_algebra_bounds(r)
    sw = ref["sum_w"]
    if sw == 0:
        return dict(grad=np.zeros_like(x), l1=0.0, ssim=0.0, loss=0.0, sum_w=0.0, cond_ok=cond_ok)
    nb = R.n_blocks(*x.shape)
    fold64 = (nb + 8) * U64
    e_sum = (N_BLOCK + 1) * U + fold64
    ws, wl = abs(ref["w_ssim"]), abs(ref["w_l1"])
    aD1, aD2, aD3 = np.abs(r["D1"]), np.abs(r["D2"]), np.abs(r["D3"])
    G = R.blur64(w * aD1) + 2 * x * R.blur64(w * aD2) + yp * R.blur64(w * aD3)
    dG = R.blur64(w * (dD1 + U * aD1)) + 2 * x * R.blur64(w * (dD2 + U * aD2)) + yp * R.blur64(w * (dD3 + U * aD3))
    grad = ws / sw * ((N_BLUR + N_OP) * U * G + dG) + N_OP * U * wl * w / sw + e_sum * (ws / sw * G + wl * w / sw)
    sum_abs_S, sum_l1 = (w * np.abs(r["S"])).sum(), (w * np.abs(x - yp)).sum()
    den = N_BLOCK * U + fold64                       # the double sum_w the scalars are divided by
    ssim = ((w * dS).sum() + ((1 + N_BLOCK) * U + fold64) * sum_abs_S) / sw + (den + U) * abs(ref["ssim"])
    l1 = ((2 + N_BLOCK) * U + fold64) * sum_l1 / sw + (den + U) * ref["l1"]
    loss = wl * l1 + ws * ssim + U * abs(ref["loss"])
    return dict(grad=grad, l1=l1, ssim=ssim, loss=loss, sum_w=e_sum * sw, cond_ok=cond_ok, G=G)
