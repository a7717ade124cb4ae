"""Restatement of the Fisher / variance entries' contract (include/r2hip.h: r2_project_gaussians_fisher,
r2_query_gaussians_variance, r2_project_gaussians_variance; csrc/gaussian_fisher.hpp), on top of the two restatements it
squares: ``gaussian_project_ref.contract`` and ``gaussian_field_ref.contract`` with G = 1 give a pair's eleven derivatives
(imported, not copied), and this module adds the squares, the weights, the variances, the sums, and the measured float32 error
the GPU tolerance is taken from.  Host only; the product never imports this file.  Scenes: ``gaussian_project_ref.SCENES``
(plus ``cone_wide`` of gaussian_project_rays_ref and an all-isotropic copy of ``cone_p7``) for the Fisher diagonal and the
projection variance, ``gaussian_field_ref.SCENES`` for the field variance.

Three quantities, each a sum of addends >= 0:

* ``fisher``  F[t, i] = sum over the pixels of w o_t^2                 (per parameter t of Gaussian i),
* ``pvar``    out[pixel] = sum over the Gaussians of sum_t v[t, i] o_t^2   (the projection variance),
* ``fvar``    out[point] = the same sum over the field's pairs             (the field variance),

in float64 twice -- ``lo``: the pairs with q <= 32, ``hi``: every pair; a sum of squares is monotone in the set of pairs, so the
contract's "a pair with q > 32 is summed or skipped" is the interval [lo, hi] -- and in float32 in the kernels' operation order
(w * (o * o); v[0] * o_0^2 first, then + v[t] * o_t^2 in ascending t; every numpy operation rounds once).

Normaliser, the same for all three: the error of a sum F is measured against  F64 + 2^-40 N,  N being the same weighted sum with
each per-pair derivative replaced by its magnitude: gauss_pair_grad's formulas with every addend replaced by its absolute value
(``magnitudes``).  A derivative that cancels analytically -- the rotation derivative of an isotropic Gaussian -- cannot be
resolved below float32's resolution of its addends, 2^-20 or so of their magnitude after a few operations, and the square of
that is the floor: 2^-40 N.  Normalising by N alone would make the test vacuous (F / N goes down to 1e-13); without the floor
the quotient is noise over noise wherever F cancels.

``measure_e32`` is the worst |f32 - f64 hi| / (F64 hi + 2^-40 N hi) per scene, quantity and group;
tests/golden/gaussian_fisher/e32.json holds it (written by ``python -m tests.gaussian_fisher_ref``); the GPU tests allow 4 x
that, plus gaussian_project_ref.FLOOR.
"""
import json
import os

import numpy as np

from tests import gaussian_field_ref as RF
from tests import gaussian_project_ref as RP

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gaussian_fisher", "e32.json")
GROUPS = RP.GRADS                                   # xyz, density, scaling, rotation
ROWS = {"xyz": slice(0, 3), "density": slice(3, 4), "scaling": slice(4, 7), "rotation": slice(7, 11)}
FLOOR = RP.FLOOR
FLOOR_BITS = 2.0 ** -40
# per-group constants of the scenes' variances: a hundredth of the cloud's extent for lengths, a tenth for the rest
VAR_SCALE = {"xyz": 1e-4, "density": 1e-2, "scaling": 1e-4, "rotation": 1e-2}

PROJ_SCENES = tuple(RP.SCENES) + ("cone_wide", "cone_p7_iso")
FIELD_SCENES = tuple(RF.SCENES)
IDENTITY_SCENES = ("cone_p7", "parallel_p300", "cone_stack300")


# ------------------------------------------------------------------------------------------------------ scenes
def proj_scene(name):
    if name == "cone_wide":
        from tests import gaussian_project_rays_ref as RR
        return RR.scene(name)
    if name == "cone_p7_iso":   # every Gaussian isotropic: d term / d quaternion is analytically 0
        sc = RP.scene("cone_p7")
        xyz, dens, scal, rot = sc["cloud"]
        return dict(sc, cloud=(xyz, dens, np.repeat(scal[:, :1], 3, 1).copy(), rot))
    return RP.scene(name)


def scene_weights(V, H, W):
    """[V,H,W] float32 in [0.5, 1.5), fixed seed."""
    return (0.5 + np.random.RandomState(71).rand(V, H, W)).astype(np.float32)


def scene_variances(P):
    """{group: [P, c] float32}: (0.5 + 1.5 rand) x VAR_SCALE[group], fixed seed.  Not derived from any Fisher diagonal, so the
    variance entries are tested independently of the Fisher entry."""
    g = np.random.RandomState(72)
    return {k: ((0.5 + 1.5 * g.rand(P, ROWS[k].stop - ROWS[k].start)) * VAR_SCALE[k]).astype(np.float32) for k in GROUPS}


def stack(d, dtype):
    """{group: [P, c]} -> [11, P] in `dtype`."""
    return np.concatenate([np.asarray(d[k], np.float32).reshape(-1, ROWS[k].stop - ROWS[k].start).T for k in GROUPS], 0).astype(dtype)


# ------------------------------------------------------------------------------------------------------ magnitudes
def magnitudes(M, isg, e, d, u, w, wp, A, k, t0, length, rho, scale, quat):
    """gauss_pair_grad's eleven formulas (csrc/gaussian_rays.hpp) with G = 1 and every addend replaced by its absolute value:
    what each derivative would be if nothing in it cancelled.  The arguments are gauss_pair's quantities as the contract
    computes them (a point: d = u = 0, A = 1, k = 0, wp = w, |d| = 1)."""
    a = np.abs
    T = a(rho) * t0
    gw = [T * a(wp[i]) for i in range(3)]
    gu = [T * (a(k) * a(wp[i]) + a(u[i]) / A) for i in range(3)]
    hu = [gu[i] * a(isg[i]) for i in range(3)]
    hw = [gw[i] * a(isg[i]) for i in range(3)]
    m = [length * (a(M[0][j]) * gw[0] + a(M[1][j]) * gw[1] + a(M[2][j]) * gw[2]) for j in range(3)]
    m.append(t0 * length)
    m += [length * ((gu[i] * a(u[i]) + gw[i] * a(w[i])) / a(scale[i])) for i in range(3)]
    D = [[length * (a(d[j]) * hu[i] + a(e[j]) * hw[i]) for i in range(3)] for j in range(3)]
    r, x, y, z = (a(c) for c in quat)
    m.append(2.0 * (z * (D[1][0] + D[0][1]) + y * (D[0][2] + D[2][0]) + x * (D[2][1] + D[1][2])))
    m.append(2.0 * (y * (D[0][1] + D[1][0]) + z * (D[0][2] + D[2][0]) + r * (D[2][1] + D[1][2])) + 4.0 * (x * (D[1][1] + D[2][2])))
    m.append(2.0 * (x * (D[0][1] + D[1][0]) + r * (D[0][2] + D[2][0]) + z * (D[1][2] + D[2][1])) + 4.0 * (y * (D[0][0] + D[2][2])))
    m.append(2.0 * (r * (D[1][0] + D[0][1]) + x * (D[0][2] + D[2][0]) + y * (D[1][2] + D[2][1])) + 4.0 * (z * (D[0][0] + D[1][1])))
    return m


def _ray_magnitudes(s, d, mu, rho, scale, mod, quat):
    """The quantities of gauss_pair for all pairs (float64), handed to ``magnitudes``.  They are the first lines of
    gaussian_project_ref.contract, which returns the derivatives but not what they are made of."""
    Rm = RP._rot(quat)
    isg = [1.0 / (scale[i] * mod) for i in range(3)]
    M = [[Rm[j][i] * isg[i] for j in range(3)] for i in range(3)]
    e = [s[j] - mu[j] for j in range(3)]
    u = [M[i][0] * d[0] + M[i][1] * d[1] + M[i][2] * d[2] for i in range(3)]
    w = [M[i][0] * e[0] + M[i][1] * e[1] + M[i][2] * e[2] for i in range(3)]
    A = u[0] * u[0] + u[1] * u[1] + u[2] * u[2]
    k = (u[0] * w[0] + u[1] * w[1] + u[2] * w[2]) / A
    wp = [w[i] - k * u[i] for i in range(3)]
    q = wp[0] * wp[0] + wp[1] * wp[1] + wp[2] * wp[2]
    t0 = np.sqrt(RP.TWO_PI / A) * np.exp(-0.5 * q)
    length = np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
    return magnitudes(M, isg, e, d, u, w, wp, A, k, t0, length, rho, scale, quat)


def _point_magnitudes(x, mu, rho, scale, mod, quat):
    Rm = RP._rot(quat)
    isg = [1.0 / (scale[i] * mod) for i in range(3)]
    M = [[Rm[j][i] * isg[i] for j in range(3)] for i in range(3)]
    e = [x[j] - mu[j] for j in range(3)]
    w = [M[i][0] * e[0] + M[i][1] * e[1] + M[i][2] * e[2] for i in range(3)]
    q = w[0] * w[0] + w[1] * w[1] + w[2] * w[2]
    zero = [0.0, 0.0, 0.0]
    return magnitudes(M, isg, e, zero, zero, w, w, 1.0, 0.0, np.exp(-0.5 * q), 1.0, rho, scale, quat)


# ------------------------------------------------------------------------------------------------------ the sums
PIECE = 1 << 19   # pairs per piece (memory)


def _accumulate(o, masks, wv, v, msq, res, idx):
    """One piece of pairs [n, P].  o: the eleven derivatives (0 where the pair is not summed); masks: one [n, P] bool or None
    (every pair of o) per limit; wv [n, 1] weights or None; v [11, P]; msq: the eleven squared magnitudes or None."""
    for b, mask in enumerate(masks):
        pv = npv = None
        for t in range(11):
            sq = o[t] * o[t]
            if mask is not None:
                sq = np.where(mask, sq, np.zeros_like(sq))
            if wv is not None:
                res["F"][b][t] += (wv * sq).sum(0)
            term = v[t][None, :] * sq
            pv = term if pv is None else pv + term
            if msq is not None:
                ms = msq[t] if mask is None else np.where(mask, msq[t], 0.0)
                if wv is not None:
                    res["NF"][b][t] += (wv * ms).sum(0)
                nt = v[t][None, :] * ms
                npv = nt if npv is None else npv + nt
        res["pv"][b][idx] = pv.sum(1)
        if msq is not None:
            res["Npv"][b][idx] = npv.sum(1)


def _new(nlim, P, N, dtype):
    return {"F": [np.zeros((11, P), dtype) for _ in range(nlim)], "NF": [np.zeros((11, P), np.float64) for _ in range(nlim)],
            "pv": [np.zeros(N, dtype) for _ in range(nlim)], "Npv": [np.zeros(N, np.float64) for _ in range(nlim)]}


def projector_sums(dtype, rays, cone, H, W, xyz, density, scaling, rotation, mod, weights, var):
    """float64: both limits (index 0: q <= 32, index 1: every pair) with their normalisers; float32: every pair, no normaliser.
    -> dict(F, NF: lists of [11, P]; pv, Npv: lists of [V, H, W])."""
    f64 = dtype == np.float64
    V, P = np.asarray(rays).shape[0], np.asarray(xyz).shape[0]
    S, Dr = RP.pixel_rays(rays, cone, H, W, dtype)
    mu, sc, qt = RP._cols(xyz, dtype), RP._cols(scaling, dtype), RP._cols(rotation, dtype)
    rho = RP._cols(np.asarray(density).reshape(P, 1), dtype)[0]
    v = stack(var, dtype)
    res = _new(2 if f64 else 1, P, V * H * W, dtype)
    step = max(1, PIECE // max(P, 1))
    with np.errstate(all="ignore"):
        for view in range(V):
            for a in range(0, H * W, step):
                s = [S[j][view].reshape(-1, 1)[a:a + step] for j in range(3)]
                d = [Dr[j][view].reshape(-1, 1)[a:a + step] for j in range(3)]
                wv = np.asarray(weights, np.float32).astype(dtype)[view].reshape(-1, 1)[a:a + step]
                o = RP.contract(np, s, d, cone, mu, rho, sc, dtype(mod), qt, None, np.ones_like(s[0]))
                msq = None
                if f64:
                    msq = [np.where(o["keep"], m * m, 0.0) for m in _ray_magnitudes(s, d, mu, rho, sc, dtype(mod), qt)]
                masks = [o["keep"] & (o["q"] <= 32.0), None] if f64 else [None]
                idx = slice(view * H * W + a, view * H * W + a + s[0].shape[0])
                _accumulate(o["grads"], masks, wv, v, msq, res, idx)
    for k in ("pv", "Npv"):
        res[k] = [x.reshape(V, H, W) for x in res[k]]
    return res


def field_sums(dtype, points, xyz, density, scaling, rotation, mod, var):
    """The field variance at every point: as ``projector_sums``, without weights.  -> dict(pv, Npv: lists of [N])."""
    f64 = dtype == np.float64
    pts = np.asarray(points, np.float32).reshape(-1, 3).astype(dtype)
    N, P = pts.shape[0], np.asarray(xyz).shape[0]
    res = _new(2 if f64 else 1, P, N, dtype)
    if P == 0:
        return res
    mu, sc, qt = RP._cols(xyz, dtype), RP._cols(scaling, dtype), RP._cols(rotation, dtype)
    rho = RP._cols(np.asarray(density).reshape(P, 1), dtype)[0]
    v = stack(var, dtype)
    step = max(1, PIECE // P)
    with np.errstate(all="ignore"):
        for a in range(0, N, step):
            x = [pts[a:a + step, j:j + 1] for j in range(3)]
            o = RF.contract(np, x, mu, rho, sc, dtype(mod), qt, None, None, np.ones_like(x[0]))
            msq = None
            if f64:
                msq = [np.where(o["keep"], m * m, 0.0) for m in _point_magnitudes(x, mu, rho, sc, dtype(mod), qt)]
            masks = [o["keep"] & (o["q"] <= 32.0), None] if f64 else [None]
            _accumulate(o["grads"][:11], masks, None, v, msq, res, slice(a, a + x[0].shape[0]))
    return res


# ------------------------------------------------------------------------------------------------------ references
_CACHE = {}


def _proj_inputs(name):
    sc = proj_scene(name)
    V, P = sc["rays"].shape[0], sc["cloud"][0].shape[0]
    return sc, scene_weights(V, sc["H"], sc["W"]), scene_variances(P)


def projector_reference(name):
    """Float64 sums of a projector scene, computed once per process: dict(scene, weights, var, F, NF, pv, Npv; lists are
    [lo, hi]), and T, NT: the totals sum_it F v and their normalisers, [lo, hi]."""
    key = ("proj", name)
    if key not in _CACHE:
        sc, wts, var = _proj_inputs(name)
        r = projector_sums(np.float64, sc["rays"], sc["cone"], sc["H"], sc["W"], *sc["cloud"], sc["mod"], wts, var)
        v = stack(var, np.float64)
        r.update(scene=sc, weights=wts, var=var, T=[float((F * v).sum()) for F in r["F"]], NT=[float((F * v).sum()) for F in r["NF"]])
        _CACHE[key] = r
    return _CACHE[key]


def field_reference(name):
    key = ("field", name)
    if key not in _CACHE:
        sc = RF.scene(name)
        var = scene_variances(sc["cloud"][0].shape[0])
        r = field_sums(np.float64, sc["points"], *sc["cloud"], sc["mod"], var)
        r.update(scene=sc, var=var)
        _CACHE[key] = r
    return _CACHE[key]


# The end-to-end case: the cloud and the three training views of cone_p7 (angles 0.3 + 2.1 i), prior precision 1e-3, four
# candidate views: training view 0 again, that view rotated by 90 degrees, training view 1 again, and one in between.
END_TO_END = {"scene": "cone_p7", "prior": 1e-3, "angles": (0.3, 0.3 + np.pi / 2, 2.4, 1.2), "seen": 0, "unseen": 1}


def candidate_views(name=END_TO_END["scene"], angles=END_TO_END["angles"]):
    """scene.View list at `angles` with the detector and geometry of the projector scene `name` (gaussian_project_ref._views)."""
    from r2_gaussian_amd import scene as S
    sc = proj_scene(name)
    cfg = dict(S.CONE_BEAM, mode=name.split("_", 1)[0], DSO=5.0, DSD=7.0)
    return [S.make_view(a, (sc["H"], sc["W"]), cfg) for a in angles]


def information64():
    """view_information of the end-to-end case in float64, every pair, unit weights: -> [4] scores."""
    from r2_gaussian_amd import projector
    sc = proj_scene(END_TO_END["scene"])
    P = sc["cloud"][0].shape[0]
    ones = lambda V: np.ones((V, sc["H"], sc["W"]), np.float32)
    zero = {k: np.zeros((P, ROWS[k].stop - ROWS[k].start), np.float32) for k in GROUPS}
    F = projector_sums(np.float64, sc["rays"], sc["cone"], sc["H"], sc["W"], *sc["cloud"], sc["mod"], ones(len(sc["views"])), zero)["F"][1]
    var = 1.0 / (F + END_TO_END["prior"])
    rays = projector.ray_params(candidate_views(), (1.0, 1.0, 1.0), (0.0, 0.0, 0.0), (1, 1, 1))
    return np.array([(projector_sums(np.float64, rays[i:i + 1], sc["cone"], sc["H"], sc["W"], *sc["cloud"], sc["mod"], ones(1),
                                     zero)["F"][1] * var).sum() for i in range(rays.shape[0])])


def normaliser(F, N):
    return F + FLOOR_BITS * N


def _worst(got, F, N):
    den = normaliser(F, N)
    m = den > FLOOR
    return float((np.abs(np.asarray(got, np.float64).reshape(F.shape) - F)[m] / den[m]).max()) if m.any() else 0.0


def measure_projector_e32(name):
    """-> ({group: e32 of the Fisher diagonal}, e32 of the projection variance)."""
    r = projector_reference(name)
    sc = r["scene"]
    f32 = projector_sums(np.float32, sc["rays"], sc["cone"], sc["H"], sc["W"], *sc["cloud"], sc["mod"], r["weights"], r["var"])
    return {k: _worst(f32["F"][0][ROWS[k]], r["F"][1][ROWS[k]], r["NF"][1][ROWS[k]]) for k in GROUPS}, \
        _worst(f32["pv"][0], r["pv"][1], r["Npv"][1])


def measure_field_e32(name):
    r = field_reference(name)
    sc = r["scene"]
    f32 = field_sums(np.float32, sc["points"], *sc["cloud"], sc["mod"], r["var"])
    return _worst(f32["pv"][0], r["pv"][1], r["Npv"][1])


def measure_e32():
    out = {"fisher": {}, "projection_variance": {}, "field_variance": {}}
    for n in PROJ_SCENES:
        out["fisher"][n], out["projection_variance"][n] = measure_projector_e32(n)
    for n in FIELD_SCENES:
        out["field_variance"][n] = measure_field_e32(n)
    return out


def load_e32():
    with open(GOLDEN) as f:
        return json.load(f)


def bracket(got, F, N, e32, what):
    """Assert got inside [F lo - tol lo, F hi + tol hi], tol = 4 e32 (F + 2^-40 N) + FLOOR of each limit; F, N: [lo, hi].
    Prints and returns the worst excess in units of the tolerance."""
    got = np.asarray(got, np.float64).reshape(F[0].shape)
    tol = [4.0 * e32 * normaliser(F[b], N[b]) + FLOOR for b in range(2)]
    lo, hi = F[0] - tol[0], F[1] + tol[1]
    bad = (got < lo) | (got > hi) | ~np.isfinite(got)
    worst = float(np.max(np.maximum((lo - got) / tol[0], (got - hi) / tol[1]))) if got.size else -1.0
    print("%s: worst excess over the bracket in units of the tolerance %.3f (<= 0 passes)" % (what, worst))
    assert not bad.any(), "%s: %d of %d outside the bracket, worst excess %.3g tolerances" % (what, int(bad.sum()), bad.size, worst)
    return worst


if __name__ == "__main__":
    os.makedirs(os.path.dirname(GOLDEN), exist_ok=True)
    res = measure_e32()
    with open(GOLDEN, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    for n, v in res["fisher"].items():
        print("fisher", n, " ".join("%s %.3e" % kv for kv in v.items()), "| projection variance %.3e" % res["projection_variance"][n])
    for n, v in res["field_variance"].items():
        print("field variance", n, "%.3e" % v)
