"""Float64 restatement of the voxelizer's render (csrc/voxel_render.hip, csrc/voxel_small.hip) with a float32 error bound.

Input: the per-Gaussian record the preprocess wrote (voxel-space mean, the 6 conic entries, opacity) and the tile lists
(point_list, ranges).  Both are pinned to the oracle elsewhere (tests/test_voxel_gpu.py: bit-exact lists, conic within 3e-7), so
what is checked against this module is the render alone.  The conic is NOT re-derived from scales and rotations: the float32
inversion of a needle's covariance is ill-conditioned, and the kernels and the oracle both start from the float32 conic.

Semantics, per (instance, voxel) pair, with d = mean - voxel centre (centres at index + 0.5):
    power = -0.5 (A dx^2 + D dy^2 + F dz^2) - B dx dy - C dx dz - E dy dz,   skipped if power > 0
    alpha = opacity exp(power),                                              skipped if alpha < 1e-6 (the float32 constant)
    vol(v) = sum of alpha over the pairs of v;   dL/dopacity(g) = sum of exp(power) dL(v) over the live pairs of g.

Error bound (u = 2^-24), the same construction as tests/projector_ref.py and tests/loss_ref.py, per voxel:

(a) Exponent rounding per pair.  Every evaluation (oracle, voxel-parallel kernels, backward) forms the exponent from float32
    products of the conic, the offsets and the log2(e)-scaled coefficients: each of its six terms t_i carries a relative error of
    a few u (d rounded: 2u for a square; coefficient scaling and the record's own rounding: 2u; an FMA chain of <= 5 steps: 5u),
    so the exponent's absolute error is <= 10 u sum|t_i| + 4 u |ln opacity| -- from the MAGNITUDES of the terms, not from their
    sum, so the cancellation of a thin Gaussian's terms is covered.  exp / exp2 (1 ulp) and the opacity product add 8 u relative.
    Entries the lane-per-entry step may serve (not needs_exact_slab3) reach a voxel (row offset j <= 3 from its anchor row 4 or
    3, z offset c <= 3 from its segment start 0 or 4) through a product of exp2 values: the anchor 2^E(anchor), j row ratios
    (their argument E(y+1) - E(y), built from 2^(E(5) - E(4)) and j(j-1)/2 factors kappa = 2^(2 d2)), c z ratios (from
    2^(E(z+1) - E(z)) and the factors chi = 2^e2, rr = 2^(2 f2): j c and c(c-1)/2 of them).  Each argument is again an FMA chain
    of magnitudes: with M_a the anchor's term magnitudes (+|L|), M_r = 0.5|D|(1 + 2|dy_a|) + |B dx| + |E dz_s| and
    M_t = 0.5|F|(1 + 2|dz_s|) + |E dy_a| + |C dx| the two ratios', the exponent reaching the voxel is off by at most
        12 u (M_a + j M_r + c M_t + j(j-1)/2 |D| + j c |E| + c(c-1)/2 |F|)
    and the chain's <= 25 exp2 values (2u each) and <= 30 products (u each) add 80 u relative.  With delta the pair's total
    exponent error (natural-log units), its value is within expm1(delta) alpha of the float64 alpha.
(b) Summation.  Whatever the order (lane accumulators, the 64 x 64 transpose-reduction, the voxel-parallel tail, the combine of
    a tile's work items, the oracle's sequential loop), a sum of m non-zero terms is off by at most gamma_m = m u / (1 - m u)
    times the sum of their magnitudes (adding the zeros of culled pairs is exact).
(c) The cut-off band.  A pair whose float64 log alpha lies within its own delta of log(1e-6), or whose power lies within its
    own rounding error (10 u sum|t_i|, plus 2 u |ln opacity| unless every term is 0) of 0, may be in or out in float32: its whole alpha (times 1 + expm1(delta)) goes into the bound, and into the count m of (b).

dL/dopacity gets the same three terms with the backward's exact exponent (no recurrence) and the product with dL (u).

The bound is useful only if it is tight: `tightness` reports, per voxel, whether the bound is below the smallest contribution
outside the band -- where it is, dropping or duplicating any single pair breaks the check.

Also here: the float32 restatement of the culling record and of the two tier rules (needs_exact_slab3, slab_live), shared with
tests/test_voxel_slab_math_cpu.py.
"""
import numpy as np

LOG2E = 1.4426950408889634
LN2 = 0.6931471805599453
LOG2_ALPHA_MIN = -19.931568569324174
ALPHA_MIN = 1e-6
ALPHA_MIN32 = float(np.float32(1e-6))   # the kernels' and the oracle's 0.000001f
U = 2.0 ** -24
f32 = np.float32


# ------------------------------------------------------------------------------------------------ the culling record, tier rules
def record(mean, conic, op):
    """What voxel_preprocess_one stores: float32 record + culling extents (computed in double from the float32 conic).
    conic: [n,3,3] inverse covariances (voxel units), or [n,6] (xx, xy, xz, yy, yz, zz)."""
    conic = np.asarray(conic)
    if conic.ndim == 2:
        conic = conic6_to_33(conic)
    A, B, C, D, E, F = (conic[:, 0, 0].astype(f32).astype(np.float64), conic[:, 0, 1].astype(f32).astype(np.float64),
                        conic[:, 0, 2].astype(f32).astype(np.float64), conic[:, 1, 1].astype(f32).astype(np.float64),
                        conic[:, 1, 2].astype(f32).astype(np.float64), conic[:, 2, 2].astype(f32).astype(np.float64))
    with np.errstate(all="ignore"):
        L = np.log2(np.asarray(op).astype(f32)).astype(f32)
    qmax = 2.0 * LN2 * (L.astype(np.float64) - LOG2_ALPHA_MIN) + 1e-3
    m00, m11, m22 = D * F - E * E, A * F - C * C, A * D - B * B
    det3 = A * m00 - B * (B * F - C * E) + C * (B * E - C * D)
    ok = (qmax > 0) & (A > 0) & (m22 > 0) & (det3 > 0) & (m00 > 0) & (m11 > 0) & (D > 0) & (F > 0) & \
         ((A + D + F) * (m00 + m11 + m22) <= 1.0e4 * det3)
    with np.errstate(all="ignore"):
        hx = np.where(ok, np.sqrt(qmax * m00 / det3) * 1.004 + 0.05, np.inf)
        hyc = np.where(ok, np.sqrt(qmax * F / m00) * 1.004 + 0.05, np.inf)
        hzc = np.where(ok, np.sqrt(qmax * D / m00) * 1.004 + 0.05, np.inf)
        ky = np.where(ok, -(F * B - E * C) / m00, 0.0)
        kz = np.where(ok, -(D * C - E * B) / m00, 0.0)
    dead = ~(qmax > 0)
    hx, hyc, hzc = (np.where(dead, -np.inf, h) for h in (hx, hyc, hzc))
    rec = dict(p=np.asarray(mean).astype(f32),
               a2=(f32(-0.5 * LOG2E) * A.astype(f32)), b2=(f32(-LOG2E) * B.astype(f32)), c2=(f32(-LOG2E) * C.astype(f32)),
               d2=(f32(-0.5 * LOG2E) * D.astype(f32)), e2=(f32(-LOG2E) * E.astype(f32)), f2=(f32(-0.5 * LOG2E) * F.astype(f32)),
               L=L, hx=hx.astype(f32), hyc=hyc.astype(f32), hzc=hzc.astype(f32), ky=ky.astype(f32), kz=kz.astype(f32), safe=ok)
    return rec


def conic6_to_33(c6):
    c6 = np.asarray(c6)
    a, b, c, d, e, f = (c6[:, i] for i in range(6))
    return np.stack([a, b, c, b, d, e, c, e, f], 1).reshape(-1, 3, 3)


def slab_live(rec, xc, y0=0.0, z0=0.0):
    """csrc/voxel_render.hip: slab_live, in float32 (slab x = xc of the tile whose voxel rows start at y0, z0)."""
    p = rec["p"]
    with np.errstate(all="ignore"):
        dx = p[:, 0] - f32(xc)
        u = dx * (f32(1.0) / rec["hx"])
        t = np.sqrt(np.maximum(f32(1.0) - u * u, f32(0.0))).astype(f32)
        cy, cz = p[:, 1] - rec["ky"] * dx, p[:, 2] - rec["kz"] * dx
        ey, ez = rec["hyc"] * t, rec["hzc"] * t
        return (np.abs(dx) <= rec["hx"]) & (cy - ey <= f32(y0 + 7.5)) & (cy + ey >= f32(y0 + 0.5)) & \
               (cz - ez <= f32(z0 + 7.5)) & (cz + ez >= f32(z0 + 0.5))


def needs_exact(rec, margin=1.0):
    """voxel_state.hpp: needs_exact_slab3 (VOX_RECUR_YSTEPS = 3, VOX_RECUR_STEPS - 1 = 3).  margin > 1 lets entries up to
    (margin - 1) beyond the rule's threshold count as stepped too (a record restated from a rounded conic can sit on the other
    side of it)."""
    L = rec["L"]
    with np.errstate(all="ignore"):
        smax = np.sqrt(np.maximum(f32(125.5) + np.minimum(L, f32(0)), f32(0))) - np.sqrt(np.maximum(L - f32(LOG2_ALPHA_MIN), f32(0)) + f32(1))
        need = f32(3) * np.sqrt(np.abs(rec["d2"])) + f32(3) * np.sqrt(np.abs(rec["f2"]))
    return ~((smax > 0) & (need <= f32(margin) * smax)) | ~(rec["hx"] < f32(3.0e38))


# ------------------------------------------------------------------------------------------------ the float64 render
def tiles_of_instances(ranges, R):
    lengths = ranges[:, 1].astype(np.int64) - ranges[:, 0].astype(np.int64)
    assert (lengths >= 0).all() and lengths.sum() == R, "ranges do not partition the list"
    return np.repeat(np.arange(ranges.shape[0], dtype=np.int64), lengths)


def gamma(m):
    m = np.asarray(m, np.float64)
    return m * U / (1.0 - m * U)


def render(means, conic6, opacity, point_list, ranges, nVoxel, voxels=None, dL=None, sVoxel=None, max_pairs=1 << 20):
    """Float64 volume and dL/dopacity with their float32 error bounds.

    means [P,3], conic6 [P,6], opacity [P] (the float32 record); point_list, ranges: the tile lists of the grid nVoxel.
    voxels: flat indices (x * ny + y) * nz + z of the voxels to evaluate (None: all).  dL: [nx, ny, nz] or None.
    -> dict(voxels, value, bound [float32, rounded up], n_pairs (live + band), min_out (smallest live contribution outside the
       band, +inf if none), n_band; with dL: dop, dop_bound, dop_pairs, dop_min_w (smallest live |G dL| outside the band);
       with dL and sVoxel also dmean, dmean_bound [P,3] (dL/dmeans3D) and raw [P,10] (the float64 sums of VOXEL_RAW order:
       dL/dmean3D_norm, dL/dconic3D, dL/dopacity -- what the geometry chain starts from))."""
    means = np.asarray(means, np.float32).reshape(-1, 3).astype(np.float64)
    c6 = np.asarray(conic6, np.float32).reshape(-1, 6).astype(np.float64)
    op32 = np.asarray(opacity, np.float32).reshape(-1)
    op = op32.astype(np.float64)
    P = means.shape[0]
    nx, ny, nz = (int(k) for k in nVoxel)
    gx, gy, gz = (nx + 7) // 8, (ny + 7) // 8, (nz + 7) // 8
    T = gx * gy * gz
    point_list = np.asarray(point_list).astype(np.int64)
    ranges = np.asarray(ranges).reshape(T, 2)
    R = point_list.size
    tiles = tiles_of_instances(ranges, R)
    voxels = np.arange(nx * ny * nz, dtype=np.int64) if voxels is None else np.asarray(voxels, np.int64)
    nv = voxels.size
    vz_all = voxels % nz
    vy_all = (voxels // nz) % ny
    vx_all = voxels // (ny * nz)
    vt = (vz_all // 8 * gy + vy_all // 8) * gx + vx_all // 8
    vorder = np.argsort(vt, kind="stable")
    vcount = np.bincount(vt, minlength=T)
    vstart = np.cumsum(vcount) - vcount
    # entries the lane-per-entry step may serve (restated tier rule, with a margin: the restated record is rounded once more)
    with np.errstate(all="ignore"):
        stepped_g = ~needs_exact(record(means.astype(np.float32), c6.astype(np.float32), op32), margin=1.01) & (op > 0)
    lncut = np.log(ALPHA_MIN32)

    value = np.zeros(nv)
    err = np.zeros(nv)
    absum = np.zeros(nv)
    npairs = np.zeros(nv)
    nband = np.zeros(nv)
    min_out = np.full(nv, np.inf)
    if dL is not None:
        dLf = np.asarray(dL, np.float32).reshape(-1).astype(np.float64)
        dop, dop_err, dop_abs, dop_n = np.zeros(P), np.zeros(P), np.zeros(P), np.zeros(P)
        dop_min_w = np.full(P, np.inf)
        # the backward's ten moments of w = G dL per Gaussian: sum w, sum w d_j, sum w d_j d_k (xx xy xz yy yz zz), their
        # error (rounding of each term + the band) and their magnitude (for the summation term)
        mom, mom_err, mom_abs = np.zeros((10, P)), np.zeros((10, P)), np.zeros((10, P))

    nper = vcount[tiles]
    cum = np.cumsum(nper)
    k0 = 0
    while k0 < R:
        k1 = int(np.searchsorted(cum, (cum[k0 - 1] if k0 else 0) + max_pairs, side="right"))
        k1 = max(k1, k0 + 1)
        cnt = nper[k0:k1]
        tot = int(cnt.sum())
        if tot == 0:
            k0 = k1
            continue
        inst = np.repeat(np.arange(k0, k1), cnt)
        within = np.arange(tot) - np.repeat(np.cumsum(cnt) - cnt, cnt)
        slot = vorder[vstart[tiles[inst]] + within]            # index into `voxels`
        gid = point_list[inst]
        vx, vy, vz = vx_all[slot], vy_all[slot], vz_all[slot]
        p = means[gid]
        dx, dy, dz = p[:, 0] - (vx + 0.5), p[:, 1] - (vy + 0.5), p[:, 2] - (vz + 0.5)
        A, B, C, D, E, F = (c6[gid, i] for i in range(6))
        o = op[gid]
        ta, td, tf = 0.5 * A * dx * dx, 0.5 * D * dy * dy, 0.5 * F * dz * dz
        tb, tc, te = B * dx * dy, C * dx * dz, E * dy * dz
        power = -(ta + td + tf + tb + tc + te)
        mag = np.abs(ta) + np.abs(td) + np.abs(tf) + np.abs(tb) + np.abs(tc) + np.abs(te)
        with np.errstate(divide="ignore"):
            lnop = np.log(o)
        pos = o > 0
        lnop = np.where(pos, lnop, 0.0)
        # (a) exponent error, exact evaluation (natural-log units)
        de = U * (10.0 * mag + 4.0 * np.abs(lnop) + 8.0)
        # ... and the recurrence of the lane-per-entry step
        st = stepped_g[gid]
        yl, zl = vy % 8, vz % 8
        ya = np.where(yl >= 4, 4, 3)
        j = np.abs(yl - ya)
        seg = np.where(zl >= 4, 4, 0)
        c = zl - seg
        dya = p[:, 1] - (vy - yl + ya + 0.5)
        dzs = p[:, 2] - (vz - zl + seg + 0.5)
        aA, aB, aC, aD, aE, aF = np.abs(A), np.abs(B), np.abs(C), np.abs(D), np.abs(E), np.abs(F)
        adx, adya, adzs = np.abs(dx), np.abs(dya), np.abs(dzs)
        Ma = 0.5 * aA * dx * dx + aB * adx * adya + aC * adx * adzs + 0.5 * aD * dya * dya + aE * adya * adzs + \
            0.5 * aF * dzs * dzs + np.abs(lnop)
        Mr = 0.5 * aD * (1.0 + 2.0 * adya) + aB * adx + aE * adzs
        Mt = 0.5 * aF * (1.0 + 2.0 * adzs) + aE * adya + aC * adx
        small = 0.5 * j * (j - 1) * aD + j * c * aE + 0.5 * c * (c - 1) * aF
        dr = U * (12.0 * (Ma + j * Mr + c * Mt + small) + 80.0)
        delta = de + np.where(st, dr, 0.0)
        rel = np.expm1(delta)
        lna = power + lnop
        alpha = np.where(pos, np.exp(np.minimum(lna, 700.0)), 0.0)
        live = pos & (power <= 0.0) & (alpha >= ALPHA_MIN32)
        # (the power > 0 test: the error of power alone -- exactly 0 at a voxel on the centre, where every term is 0)
        dp = U * (10.0 * mag + 2.0 * np.abs(lnop) * (mag > 0))
        band = pos & ((np.abs(lna - lncut) <= delta) | ((np.abs(power) < dp) & (lna >= lncut - delta)))
        certain = live & ~band
        counted = live | band
        w_val = np.where(live, alpha, 0.0)
        value += np.bincount(slot, w_val, minlength=nv)
        err += np.bincount(slot, np.where(certain, alpha * rel, 0.0) + np.where(band, alpha * (1.0 + rel), 0.0), minlength=nv)
        absum += np.bincount(slot, np.where(counted, alpha * (1.0 + rel), 0.0), minlength=nv)
        npairs += np.bincount(slot, counted.astype(np.float64), minlength=nv)
        nband += np.bincount(slot, band.astype(np.float64), minlength=nv)
        np.minimum.at(min_out, slot[certain], alpha[certain])
        if dL is not None:
            # backward: exact exponent (no recurrence), G = exp(power), the same cut-off on opacity * G
            bband = pos & ((np.abs(lna - lncut) <= de) | ((np.abs(power) < dp) & (lna >= lncut - de)))
            G = np.exp(np.minimum(power, 700.0))
            w = G * dLf[voxels[slot]]
            relb = np.expm1(de) + U
            bcount = live | bband
            dop += np.bincount(gid, np.where(live, w, 0.0), minlength=P)
            dop_err += np.bincount(gid, np.where(live & ~bband, np.abs(w) * relb, 0.0) +
                                   np.where(bband, np.abs(w) * (1.0 + relb), 0.0), minlength=P)
            dop_abs += np.bincount(gid, np.where(bcount, np.abs(w) * (1.0 + relb), 0.0), minlength=P)
            dop_n += np.bincount(gid, bcount.astype(np.float64), minlength=P)
            cw = live & ~bband & (w != 0.0)
            np.minimum.at(dop_min_w, gid[cw], np.abs(w[cw]))
            if sVoxel is not None:
                # d as the kernel forms it (voxel offsets from a tile origin): absolute error <= u (|d| + 9)
                d = (dx, dy, dz)
                de_ = [U * (np.abs(t) + 9.0) for t in d]
                ms = [(np.ones_like(dx), np.zeros_like(dx))] + [(d[j], de_[j]) for j in range(3)] + \
                     [(d[j] * d[k], np.abs(d[k]) * de_[j] + np.abs(d[j]) * de_[k]) for j, k in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))]
                aw = np.abs(w)
                for q, (m, me) in enumerate(ms):
                    am = np.abs(m)
                    mom[q] += np.bincount(gid, np.where(live, w * m, 0.0), minlength=P)
                    mom_err[q] += np.bincount(gid, np.where(live & ~bband, aw * (am * (relb + 2.0 * U) + me), 0.0) +
                                              np.where(bband, aw * (am * (1.0 + relb) + me), 0.0), minlength=P)
                    mom_abs[q] += np.bincount(gid, np.where(bcount, aw * (am * (1.0 + relb) + me), 0.0), minlength=P)
        k0 = k1

    bound = (err + gamma(npairs) * absum) * (1.0 + 1e-3)
    out = dict(voxels=voxels, value=value, bound=_up32(bound), n_pairs=npairs.astype(np.int64), n_band=nband.astype(np.int64),
               min_out=min_out)
    if dL is not None:
        out.update(dop=dop, dop_bound=_up32((dop_err + gamma(dop_n) * dop_abs) * (1.0 + 1e-3)), dop_pairs=dop_n.astype(np.int64),
                   dop_min_w=dop_min_w)
        if sVoxel is not None:
            # csrc/voxel_geom.hip: dL/dmean3D_norm_i = opacity dv_i (-sum_j conic_ij S_j) (dv: quirk Q4), = dL/dmeans3D
            dv = np.float32(np.asarray(sVoxel, np.float32) / np.asarray(nVoxel, np.float32)).astype(np.float64)
            Cm = conic6_to_33(c6)
            S1 = mom[1:4].T                                   # [P, 3]
            E1 = (mom_err[1:4] + gamma(dop_n) * mom_abs[1:4]).T
            dmean = -op[:, None] * dv[None, :] * np.einsum("pij,pj->pi", Cm, S1)
            # conic rounding (the kernel un-scales its log2e-scaled record), three products and two sums, opacity x dv: 12 u
            dmean_bound = np.abs(op)[:, None] * dv[None, :] * (np.einsum("pij,pj->pi", np.abs(Cm), E1) +
                                                              12.0 * U * np.einsum("pij,pj->pi", np.abs(Cm), np.abs(S1)))
            raw = np.zeros((P, 10))
            raw[:, 0:3] = dmean
            raw[:, 3:9] = -op[:, None] * mom[4:10].T * np.array([0.5, 1.0, 1.0, 0.5, 1.0, 0.5])[None, :]
            raw[:, 9] = mom[0]
            out.update(dmean=dmean, dmean_bound=_up32(dmean_bound * (1.0 + 1e-3)), raw=raw)
    return out


def _up32(x):
    """float32 rounded up (never below the float64 value)."""
    y = np.asarray(x, np.float64).astype(np.float32)
    return np.where(y.astype(np.float64) < x, np.nextafter(y, np.float32(np.inf)), y).astype(np.float32)


def check(got, ref, what=""):
    """got: the voxels' float32 values (same order as ref['voxels']).  -> worst |got - value| / bound; raises on any excess."""
    got = np.asarray(got, np.float64).reshape(-1)
    e = np.abs(got - ref["value"])
    b = ref["bound"].astype(np.float64)
    bad = e > b
    if bad.any():
        i = int(np.argmax(np.where(bad, e - b, -np.inf)))
        raise AssertionError("%s: %d of %d voxels outside the float64 bound; worst voxel %d: got %.9g, float64 %.9g, |err| %.3g, "
                             "bound %.3g (%d pairs, %d in the band)" % (what, int(bad.sum()), bad.size, int(ref["voxels"][i]),
                                                                        got[i], ref["value"][i], e[i], b[i],
                                                                        ref["n_pairs"][i], ref["n_band"][i]))
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(b > 0, e / b, 0.0)
    return float(r.max()) if r.size else 0.0


def check_dop(got, ref, what=""):
    got = np.asarray(got, np.float64).reshape(-1)
    e = np.abs(got - ref["dop"])
    b = ref["dop_bound"].astype(np.float64)
    bad = e > b
    if bad.any():
        i = int(np.argmax(np.where(bad, e - b, -np.inf)))
        raise AssertionError("%s: dL/dopacity of %d of %d Gaussians outside the float64 bound; worst %d: got %.9g, float64 %.9g, "
                             "bound %.3g (%d pairs)" % (what, int(bad.sum()), bad.size, i, got[i], ref["dop"][i], b[i],
                                                        ref["dop_pairs"][i]))
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(b > 0, e / b, 0.0)
    return float(r.max()) if r.size else 0.0


def check_dmean(got, ref, what=""):
    got = np.asarray(got, np.float64).reshape(-1, 3)
    e = np.abs(got - ref["dmean"])
    b = ref["dmean_bound"].astype(np.float64)
    bad = e > b
    if bad.any():
        i = np.unravel_index(int(np.argmax(np.where(bad, e - b, -np.inf))), e.shape)
        raise AssertionError("%s: dL/dmeans3D of %d of %d Gaussians outside the float64 bound; worst %s: got %.9g, float64 %.9g, "
                             "bound %.3g" % (what, int(bad.any(1).sum()), e.shape[0], i, got[i], ref["dmean"][i], b[i]))
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(b > 0, e / b, 0.0)
    return float(r.max()) if r.size else 0.0


def tightness_dop(ref):
    """Fraction of the Gaussians holding a live pair outside the band whose dL/dopacity bound is below the smallest |G dL| of
    such a pair (where it is, a dropped or doubled backward term breaks check_dop)."""
    ne = np.isfinite(ref["dop_min_w"])
    if not ne.any():
        return 1.0, 0
    return float((ref["dop_bound"][ne].astype(np.float64) < ref["dop_min_w"][ne]).mean()), int(ne.sum())


def tightness(ref):
    """Fraction of the voxels holding a live pair outside the band whose bound is below the smallest such pair's alpha."""
    ne = np.isfinite(ref["min_out"])
    if not ne.any():
        return 1.0, 0
    return float((ref["bound"][ne].astype(np.float64) < ref["min_out"][ne]).mean()), int(ne.sum())
