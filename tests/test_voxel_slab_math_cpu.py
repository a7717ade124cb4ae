"""CPU: the arithmetic behind two round-4 changes of the voxelizer forward (csrc/voxel_render.hip, csrc/voxel_geom.hip), restated in
numpy float32 and checked against a brute-force double evaluation.  (The kernels themselves are checked against the oracle on the
GPU; this pins the two claims their comments make, over Gaussians far more extreme than the benchmark clouds hold.)

1. The cross-section slab test is CONSERVATIVE: an x-slab (1 x 8 x 8 voxels) that holds a voxel with alpha >= 1e-6 is never culled.
   Record: hx (half-width of {alpha >= 1e-6} along x), hyc / hzc (half-widths of its central y-z cross-section), ky / kz (how the
   cross-section's centre moves with x), all padded by 0.4 % + 0.05 voxel.
2. The row recurrence across the slab (rows 4..7 up from row 4, rows 3..0 down from row 3, then each row along z in two segments of
   four voxels) reproduces exp2 of the exponent for every voxel at or above the cut-off, for every Gaussian that passes
   needs_exact_slab3's bound -- in particular it never starts from an underflowed value and climbs back above the cut-off.
"""
import numpy as np
import pytest

from tests.voxel_ref import ALPHA_MIN, LOG2_ALPHA_MIN, f32, needs_exact, record, slab_live


def random_gaussians(n, seed, smin, smax):
    """-> means [n,3] (voxel units, around the tile [0,8)^3), inverse covariances [n,3,3] (double), opacities [n]."""
    rng = np.random.default_rng(seed)
    q = rng.normal(size=(n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q.T
    R = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                  2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                  2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], 1).reshape(n, 3, 3)
    s = np.exp(rng.uniform(np.log(smin), np.log(smax), size=(n, 3)))
    cov = np.einsum("nij,nj,nkj->nik", R, s * s, R)
    conic = np.linalg.inv(cov)
    mean = rng.uniform(-6.0, 14.0, size=(n, 3))
    op = np.exp(rng.uniform(np.log(2e-6), 0.0, size=n))
    return mean, conic, op


def exponent_double(rec, xc):
    """log2(alpha) of the 8 x 8 voxels of the slab x = xc of tile [0,8)^3, in double from the float32 record: [n, y, z]."""
    p = rec["p"].astype(np.float64)
    dx = (p[:, 0] - xc)[:, None, None]
    dy = p[:, 1][:, None, None] - (np.arange(8) + 0.5)[None, :, None]
    dz = p[:, 2][:, None, None] - (np.arange(8) + 0.5)[None, None, :]
    g = {k: rec[k].astype(np.float64)[:, None, None] for k in ("a2", "b2", "c2", "d2", "e2", "f2", "L")}
    return g["a2"] * dx * dx + g["b2"] * dx * dy + g["c2"] * dx * dz + g["d2"] * dy * dy + g["e2"] * dy * dz + g["f2"] * dz * dz + g["L"]


@pytest.mark.parametrize("smin,smax,seed", [(0.8, 3.0, 1), (0.25, 6.0, 2), (0.05, 12.0, 3)], ids=["ordinary", "anisotropic", "extreme"])
def test_cross_section_slab_test_never_drops_a_live_slab(smin, smax, seed):
    mean, conic, op = random_gaussians(20000, seed, smin, smax)
    rec = record(mean, conic, op)
    culled = live_total = box_total = 0
    for s in range(8):
        xc = s + 0.5
        E = exponent_double(rec, xc)
        has_live = ((E >= LOG2_ALPHA_MIN) & (E <= rec["L"].astype(np.float64)[:, None, None])).any(axis=(1, 2))
        keep = slab_live(rec, xc)
        assert not (has_live & ~keep).any(), "a slab holding a voxel above the cut-off was culled"
        culled += int((~keep).sum())
        live_total += int(has_live.sum())
        box_total += int(keep.sum())
    assert live_total > 2000, "the sample was meant to hold live slabs"
    assert box_total < 8 * len(op), "the test never culled anything"
    if smax <= 3.0:   # compact Gaussians: the cross-section test is tight (exact set / kept set)
        assert live_total >= 0.6 * box_total, (live_total, box_total)


def step_float32(rec, xc):
    """csrc/voxel_render.hip: vfwd_item's recurrences in float32 -> g[n, y, z] (the value that is compared with the cut-off)."""
    def ex2(x):
        with np.errstate(all="ignore"):
            return np.exp2(x.astype(f32)).astype(f32)
    p = rec["p"]
    q_x, q_y, q_z, q_w = rec["a2"], rec["b2"], rec["c2"], rec["d2"]
    r_x, r_y, r_z = rec["e2"], rec["f2"], rec["L"]
    n = len(r_z)
    dx = p[:, 0] - f32(xc)
    adx2L = q_x * dx * dx + r_z
    bdx, cdx = q_y * dx, q_z * dx
    dz0 = p[:, 2] - f32(0.5)
    kf1 = r_y * (f32(1.0) - f32(2.0) * dz0)
    rr, kap, chi, chii = ex2(f32(2.0) * r_y), ex2(f32(2.0) * q_w), ex2(r_x), ex2(-r_x)
    dy4, dy3 = p[:, 1] - f32(4.5), p[:, 1] - f32(3.5)
    k0u, k1u = dy4 * (q_w * dy4 + bdx) + adx2L, r_x * dy4 + cdx
    k0d, k1d = dy3 * (q_w * dy3 + bdx) + adx2L, r_x * dy3 + cdx
    eu = q_w * (f32(1.0) - f32(2.0) * dy4) - bdx
    ed = q_w * (f32(1.0) + f32(2.0) * dy3) + bdx
    out = np.zeros((n, 8, 8), f32)
    with np.errstate(all="ignore"):
        for seg in (0, 4):
            dzs = dz0 - f32(seg)
            zq, ez = r_y * dzs, r_x * dzs
            gu, gd = ex2(dzs * (zq + k1u) + k0u), ex2(dzs * (zq + k1d) + k0d)
            ru, rd = ex2(np.minimum(eu - ez, f32(100.0))), ex2(np.minimum(ed + ez, f32(100.0)))
            rtu = ex2(np.minimum(kf1 + f32(2.0 * seg) * r_y - k1u, f32(100.0)))
            rtd = (rtu * chii).astype(f32)

            def row(y, g0, rt0):
                g, rt = g0.copy(), rt0.copy()
                for c in range(4):
                    out[:, y, seg + c] = g
                    g = (g * rt).astype(f32)
                    rt = (rt * rr).astype(f32)
            for j in range(4):
                row(4 + j, gu, rtu)
                gu, ru, rtu = (gu * ru).astype(f32), (ru * kap).astype(f32), (rtu * chi).astype(f32)
            for j in range(4):
                row(3 - j, gd, rtd)
                gd, rd, rtd = (gd * rd).astype(f32), (rd * kap).astype(f32), (rtd * chii).astype(f32)
    return out


@pytest.mark.parametrize("smin,smax,seed", [(0.8, 3.0, 11), (0.3, 5.0, 12), (0.1, 8.0, 13)], ids=["ordinary", "thin", "very-thin"])
def test_row_recurrence_matches_the_exponential_wherever_the_cut_off_passes(smin, smax, seed):
    mean, conic, op = random_gaussians(20000, seed, smin, smax)
    rec = record(mean, conic, op)
    stepped = ~needs_exact(rec)                       # the entries the lane-per-entry step evaluates
    assert stepped.sum() > 1000
    errs = []
    n_live = n_false = 0
    for s in range(8):
        xc = s + 0.5
        keep = slab_live(rec, xc) & stepped
        if not keep.any():
            continue
        sub = {k: v[keep] for k, v in rec.items()}
        E = exponent_double(sub, xc)
        exact = np.exp2(E)
        g = step_float32(sub, xc).astype(np.float64)
        assert np.isfinite(g).all(), "the recurrence produced inf / NaN (0 * inf from an unclamped ratio)"
        live = E >= LOG2_ALPHA_MIN
        n_live += int(live.sum())
        if live.any():
            errs.append(np.abs(g[live] - exact[live]) / exact[live])
        # and nothing far below the cut-off is lifted above it
        far_below = exact < 0.5 * ALPHA_MIN
        n_false += int((g[far_below] >= ALPHA_MIN).sum())
    assert n_live > 20000
    err = np.concatenate(errs)
    # float32 arguments of magnitude ~100 carry ~4e-6 of relative error into each exponential, a voxel is reached through up to
    # 3 + 3 of them: the benchmark-like sample stays below 1e-5, the adversarially thin ones below 8e-5 with 99.9 % below 2e-5
    # (the parity tolerance on a voxel's SUM is 1e-4)
    assert np.median(err) < 1e-6 and np.quantile(err, 0.999) < 2e-5, (np.median(err), np.quantile(err, 0.999))
    assert err.max() < (1e-5 if smin >= 0.8 else 8e-5), "recurrence vs exp2: relative error %.3g" % err.max()
    assert n_false == 0


def test_the_bound_is_what_keeps_the_recurrence_honest():
    """Without needs_exact_slab3 the same arithmetic does lose voxels: very thin Gaussians whose anchor rows underflow."""
    mean, conic, op = random_gaussians(40000, 21, 0.05, 4.0)
    rec = record(mean, conic, op)
    flagged = needs_exact(rec) & rec["safe"] & (rec["hx"] > 0)
    assert flagged.sum() > 100
    lost = 0
    for s in range(8):
        xc = s + 0.5
        keep = slab_live(rec, xc) & flagged
        if not keep.any():
            continue
        sub = {k: v[keep] for k, v in rec.items()}
        E = exponent_double(sub, xc)
        g = step_float32(sub, xc).astype(np.float64)
        live = E >= LOG2_ALPHA_MIN + 0.01
        with np.errstate(all="ignore"):
            lost += int((live & ~(g >= 0.5 * np.exp2(E))).sum())
    assert lost > 0, "the flagged entries were meant to include cases the recurrence gets wrong"
