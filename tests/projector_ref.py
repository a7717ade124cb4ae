"""Float64 restatement of the volume forward projector (csrc/projector.hip, include/r2hip.h: r2_project_volume) and the
per-pixel float32 error bound the kernel is checked against.  Host only; the product never imports this file.

The restatement derives its rays from the views' float32 camera matrices on its own (``rays``), then evaluates the spec in
float64 from the float32 ray parameters the kernel is given (``project``), so that the only differences left are the
kernel's float32 roundings and its integer decisions.

Bound (u = 2^-24, the float32 unit roundoff; first order in u; ``SAFETY`` covers the dropped higher-order terms).  For one
pixel with ray point P = p00 + c pu + r pv, direction D and start S (cone: S = a, D = P - S; parallel: S = P, D = a):

* P: two products and two sums, |dP_a| <= 4 u (|p00_a| + c |pu_a| + r |pv_a|); cone: |dD_a| <= |dP_a| + u |D_a|;
  parallel: |dS_a| = |dP_a|.
* the slab parameters t = (B - S_a) / D_a (B = -1 or n_a): |dt| <= |t| (2 u + |dD_a| / |D_a|) + |dS_a| / |D_a|.  t0 is a
  max and t1 a min over the axes: their error is that of the largest candidate error among the axes within it of the
  extremum.
* span = t1 - t0, dt = span / n, t_k = fma(k + 1/2, dt, t0), q_k = fma(t_k, D, S):
  |d t_k| <= |dt0| + (k + 1/2)(|dspan| / n + u dt) + u |t_k|, |dq_k,a| <= |d t_k| |D_a| + |t_k| |dD_a| + |dS_a| + u |q_k,a|.
* f at q_k: Lipschitz constant 2 M_k per axis (M_k = max |vol| over the 4x4x4 voxels around the cell: any perturbed
  position stays in a neighbouring cell), plus 8 u M_k for the rounded weights (1 - w) and the three levels of weighted
  pairs (a product and an fma each).
* sum: a sequential float sum of n terms, (n - 1) u sum |f_k|; the factor dt |D_world| carries dspan / span + u
  relative from dt, 6 u + sum_a dVoxel_a |dD_a| / |D_world| from the length, and 2 u from the products.

Decisions: n = max(1, ceil(L / accuracy)) with L = span |D|: a pixel is on an n boundary when L / accuracy +- its
propagated error straddles an integer; the kernel must then match the restatement evaluated at one of the candidate n.
A pixel is on the hit/miss boundary when |span| <= |dt0| + |dt1|; the kernel may then write 0 or any value up to the
chord's largest possible integral.
"""
import numpy as np

U = 2.0 ** -24
SAFETY = 2.0


def rays(views, sVoxel, center, nVoxel):
    """[V, 12] float64 ray parameters {a, p00, pu, pv} in voxel-index coordinates, from the float32 camera matrices:
    pixel (r, c) has NDC ((2c+1)/W - 1, (2r+1)/H - 1); cone rays leave the camera centre along the view-space direction
    (ndc_x tanfovx, ndc_y tanfovy, 1), parallel rays pass view-space (ndc_x, ndc_y, 0) along +z."""
    d = np.asarray(sVoxel, np.float64) / np.asarray(nVoxel, np.float64)
    lo = np.asarray(center, np.float64) - 0.5 * np.asarray(sVoxel, np.float64)
    out = []
    for v in views:
        C2W = np.linalg.inv(v.world_view_transform.double().numpy().T)   # column vectors: world = C2W @ [view, 1]

        def to_idx_point(pv):
            return (C2W[:3, :3] @ pv + C2W[:3, 3] - lo) / d - 0.5

        def to_idx_dir(dv):
            return (C2W[:3, :3] @ dv) / d

        H, W = v.image_height, v.image_width
        ndc0 = np.array([1.0 / W - 1.0, 1.0 / H - 1.0])
        if v.mode == 1:
            tx, ty = v.tanfovx, v.tanfovy
            a = to_idx_point(np.zeros(3))
            p00 = to_idx_point(np.array([ndc0[0] * tx, ndc0[1] * ty, 1.0]))
        else:
            tx = ty = 1.0
            a = to_idx_dir(np.array([0.0, 0.0, 1.0]))
            p00 = to_idx_point(np.array([ndc0[0], ndc0[1], 0.0]))
        pu = to_idx_dir(np.array([2.0 * tx / W, 0.0, 0.0]))
        pv = to_idx_dir(np.array([0.0, 2.0 * ty / H, 0.0]))
        out.append(np.concatenate([a, p00, pu, pv]))
    return np.array(out)


def _trilinear(vol, q):
    """f(q) for q [N, 3]: trilinear, zero for neighbours outside the volume; and M = max |vol| over the 4x4x4 voxels
    around q's cell."""
    n = np.array(vol.shape)
    f0 = np.floor(q)
    w = q - f0
    i0 = f0.astype(np.int64)
    val = np.zeros(len(q))
    for dx in (0, 1):
        for dy in (0, 1):
            for dz in (0, 1):
                idx = i0 + np.array([dx, dy, dz])
                ok = ((idx >= 0) & (idx < n)).all(1)
                c = np.clip(idx, 0, n - 1)
                wt = ((w[:, 0] if dx else 1 - w[:, 0]) * (w[:, 1] if dy else 1 - w[:, 1]) * (w[:, 2] if dz else 1 - w[:, 2]))
                val += np.where(ok, vol[c[:, 0], c[:, 1], c[:, 2]], 0.0) * wt
    a = np.abs(vol)
    M = np.zeros(len(q))
    for dx in range(-1, 3):
        for dy in range(-1, 3):
            for dz in range(-1, 3):
                idx = np.clip(i0 + np.array([dx, dy, dz]), 0, n - 1)
                M = np.maximum(M, a[idx[:, 0], idx[:, 1], idx[:, 2]])
    return val, M


def _clip(S, D, n, cone):
    """-> t0, t1, error bookkeeping inputs: per-axis candidate entry/exit parameters.  S, D [R, 3]."""
    R = len(S)
    t_lo = np.full((R, 3), -np.inf)
    t_hi = np.full((R, 3), np.inf)
    inside = np.ones(R, bool)
    for ax in range(3):
        nz = D[:, ax] != 0
        with np.errstate(divide="ignore", invalid="ignore"):
            ta = (-1.0 - S[:, ax]) / D[:, ax]
            tb = (n[ax] - S[:, ax]) / D[:, ax]
        t_lo[:, ax] = np.where(nz, np.minimum(ta, tb), -np.inf)
        t_hi[:, ax] = np.where(nz, np.maximum(ta, tb), np.inf)
        inside &= nz | ((S[:, ax] > -1.0) & (S[:, ax] < n[ax]))
    t0 = t_lo.max(1)
    if cone:
        t0 = np.maximum(t0, 0.0)
    t1 = t_hi.min(1)
    return t0, t1, t_lo, t_hi, inside


def _sum_samples(vol, S, D, t0, span, nsamp):
    """sum_k f and sum_k |f|, plus the per-ray position-error accumulators, for rays with nsamp samples."""
    R = len(S)
    tot = int(nsamp.sum())
    ray = np.repeat(np.arange(R), nsamp)
    start = np.concatenate([[0], np.cumsum(nsamp)[:-1]])
    k = np.arange(tot) - np.repeat(start, nsamp)
    kk = k + 0.5
    t = t0[ray] + kk * (span[ray] / nsamp[ray])
    q = S[ray] + t[:, None] * D[ray]
    f, M = _trilinear(vol, q)
    return ray, kk, t, q, f, M


def project(vol, ray12, cone, dVoxel, accuracy, H, W, pixels=None, n_override=None):
    """Restatement on float32 ray parameters ray12 [V, 12].  pixels: optional [N, 3] (view, row, col) subset.
    -> dict(value, bound, n, n_lo, n_hi, hitmiss, cap) flattened over the pixels (row-major [V,H,W] when pixels is None).
    n_override: evaluate every hit ray with these sample counts instead (the neighbouring decision)."""
    vol = np.asarray(vol, np.float64)
    nvox = np.array(vol.shape, np.float64)
    R12 = np.asarray(ray12, np.float32).astype(np.float64)
    V = len(R12)
    if pixels is None:
        vv, rr, cc = np.meshgrid(np.arange(V), np.arange(H), np.arange(W), indexing="ij")
        pixels = np.stack([vv.ravel(), rr.ravel(), cc.ravel()], 1)
    pixels = np.asarray(pixels)
    pv = R12[pixels[:, 0]]
    r = pixels[:, 1].astype(np.float64)[:, None]
    c = pixels[:, 2].astype(np.float64)[:, None]
    P = pv[:, 3:6] + c * pv[:, 6:9] + r * pv[:, 9:12]
    eP = 4 * U * (np.abs(pv[:, 3:6]) + c * np.abs(pv[:, 6:9]) + r * np.abs(pv[:, 9:12]))
    if cone:
        S, D = pv[:, 0:3], P - pv[:, 0:3]
        eS, eD = np.zeros_like(eP), eP + U * np.abs(P - pv[:, 0:3])
    else:
        S, D = P, pv[:, 0:3]
        eS, eD = eP, np.zeros_like(eP)
    t0, t1, t_lo, t_hi, inside = _clip(S, D, nvox, cone)
    # per-axis candidate errors, and the clip points' errors
    absD = np.abs(D)
    with np.errstate(divide="ignore", invalid="ignore"):
        e_lo = np.where(np.isfinite(t_lo), np.abs(t_lo) * (2 * U + eD / absD) + eS / absD, 0.0)
        e_hi = np.where(np.isfinite(t_hi), np.abs(t_hi) * (2 * U + eD / absD) + eS / absD, 0.0)
    # an axis whose direction is within rounding of 0 (a ray parallel to a face): the kernel's candidates may swap sign
    # with D_a but stay at least `far` away; they cannot decide t0 / t1 as long as that is beyond both clip points
    far = (np.minimum(np.abs(-1.0 - S), np.abs(nvox - S)) - eS) / (absD + eD)
    reach = 2.0 * np.maximum(np.abs(np.where(np.isfinite(t0), t0, 0.0)), np.abs(np.where(np.isfinite(t1), t1, 0.0)))
    degenerate = absD <= eD
    quiet = degenerate & (far > reach[:, None])
    e_lo = np.where(quiet, 0.0, np.where(degenerate, np.inf, e_lo))
    e_hi = np.where(quiet, 0.0, np.where(degenerate, np.inf, e_hi))
    et0 = np.where(t_lo + e_lo >= t0[:, None], e_lo, 0.0).max(1)
    et1 = np.where(t_hi - e_hi <= t1[:, None], e_hi, 0.0).max(1)
    if cone:
        et0 = np.where(t0 == 0.0, 0.0, et0)
    span = t1 - t0
    hit = inside & (span > 0)
    lenD = np.sqrt((D * D).sum(1))
    elen = 3 * U * lenD + np.sqrt((eD * eD).sum(1))
    L = np.where(hit, span, 0.0) * lenD
    espan = et0 + et1 + U * np.abs(span)
    eL = espan * lenD + np.abs(span) * elen + 3 * U * L
    with np.errstate(invalid="ignore"):
        ratio = L / accuracy
        er = eL / accuracy + U * ratio
        n = np.maximum(1, np.ceil(ratio)).astype(np.int64)
        n_lo = np.maximum(1, np.ceil(ratio - er)).astype(np.int64)
        n_hi = np.maximum(1, np.ceil(ratio + er)).astype(np.int64)
    hitmiss = inside & (np.abs(span) <= et0 + et1)   # a line outside the slab of a zero-direction axis misses for both
    if n_override is not None:
        n = np.asarray(n_override, np.int64)
    n = np.where(hit, n, 0)
    # samples
    ray, kk, t, q, f, M = _sum_samples(vol, S, D, t0, np.where(hit, span, 0.0), n)
    nsafe = np.maximum(n, 1)
    sum_f = np.bincount(ray, f, minlength=len(S))
    sum_abs = np.bincount(ray, np.abs(f), minlength=len(S))
    dt = np.where(hit, span, 0.0) / nsafe
    e_dt = espan / nsafe + U * dt
    e_tk = et0[ray] + kk * e_dt[ray] + U * np.abs(t)
    e_q = (e_tk[:, None] * absD[ray] + np.abs(t)[:, None] * eD[ray] + eS[ray] + U * np.abs(q)).sum(1)
    e_f = 2.0 * M * e_q + 8 * U * M
    sum_ef = np.bincount(ray, e_f, minlength=len(S))
    dv = np.asarray(dVoxel, np.float64)
    wD = D * dv
    wlen = np.sqrt((wD * wD).sum(1))
    with np.errstate(invalid="ignore", divide="ignore"):
        e_wlen_rel = 6 * U + np.where(wlen > 0, np.sqrt(((eD * dv) ** 2).sum(1)) / wlen, 0.0)
        e_dt_rel = np.where(dt > 0, e_dt / np.where(dt > 0, dt, 1.0), 0.0)
    value = np.where(hit, dt * wlen * sum_f, 0.0)
    bound = np.where(hit, dt * wlen * (sum_ef + (nsafe + 2) * U * sum_abs) + np.abs(value) * (e_dt_rel + e_wlen_rel + 2 * U),
                     0.0) * SAFETY
    # largest possible value of a ray on the hit/miss boundary: its chord (at most et0 + et1 long) times max |vol|
    cap = (et0 + et1) * wlen * float(np.abs(vol).max(initial=0.0))
    return dict(value=value, bound=bound, n=n, n_lo=np.where(hit, n_lo, 0), n_hi=np.where(hit, n_hi, 0), hitmiss=hitmiss,
                cap=cap, hit=hit, pixels=pixels)
