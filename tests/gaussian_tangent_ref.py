"""Restatement of the Jacobian-product entries' contract (include/r2hip.h: r2_project_gaussians_jvp,
r2_project_gaussians_ray_jacobian; csrc/gaussian_tangent.hpp), on top of the restatements they apply:
``gaussian_project_ref.contract`` with G = 1 gives a pair's eleven derivatives and ``gaussian_project_rays_ref.pair_ray_grad``
with G = 1 its g_s and g_d (imported, not copied).  This module adds the tangents, the sums, the measured float32 error the GPU
tolerance is taken from, and the host loops the two Gauss-Newton solvers are held against.  Host only; the product never
imports this file.  Scenes: ``gaussian_fisher_ref.PROJ_SCENES``.

Two quantities, each a SIGNED sum over a pixel's pairs:

* ``jvp``  out[pixel] = sum over the pixel's pairs of sum_t tan[t, i] o_t        (J t),
* ``jac``  out[view, 0..5, pixel] = sum over the pixel's pairs of g_s (3), g_d (3)   (the ray Jacobian),

in float64 over every pair, and in float32 in the kernels' operation order: tan[0] * o_0 first, then + tan[t] * o_t in
ascending t; a pixel adds its pairs in ascending Gaussian index (a pair that is not summed adds an exact 0); every numpy
operation rounds once.

Normaliser of a pixel: the float64 sum over its pairs of sum_t |tan_t o_t|, for the Jacobian of |g_s|, |g_d| component by
component (two scenes add a floor: ``FLOORED_JAC``).  ``tail``: the same sum over the pairs with q > 32 alone -- the contract lets those be summed or skipped, and a
signed sum has no monotone bracket, so the tolerance carries their absolute contribution instead.

``measure_e32`` is the worst |f32 - f64| / normaliser per scene and quantity; tests/golden/gaussian_tangent/e32.json holds it
(written by ``python -m tests.gaussian_tangent_ref``, which also writes refine_lm.json and gauss_newton.json); the GPU tests
allow 4 x e32 x normaliser + tail + gaussian_project_ref.FLOOR.
"""
import json
import os

import numpy as np

from tests import gaussian_fisher_ref as RFI
from tests import gaussian_project_rays_ref as RR
from tests import gaussian_project_ref as RP

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gaussian_tangent")
GOLDEN = os.path.join(GOLDEN_DIR, "e32.json")
LM_GOLDEN = os.path.join(GOLDEN_DIR, "refine_lm.json")
GN_GOLDEN = os.path.join(GOLDEN_DIR, "gauss_newton.json")
GROUPS, ROWS, FLOOR = RFI.GROUPS, RFI.ROWS, RP.FLOOR
SCENES = RFI.PROJ_SCENES
IDENTITY_SCENES = RFI.IDENTITY_SCENES
PIECE = 1 << 19   # pairs per piece (memory)
# The ray Jacobian of these scenes is normalised as gaussian_fisher_ref normalises a sum that cancels analytically: by
# sum |g| + 2^-20 M, M the pair's magnitudes (``_ray_grad_magnitudes``).  g_d is orthogonal to d (the integral does not depend
# on |d|), and a small Gaussian seen from afar forms wp = w - k u from |w| >> |wp|: a component of a pixel's g_s or g_d can
# be orders of magnitude below the addends it is made of, and float32 cannot resolve it below 2^-20 or so of those.  Against
# sum |g| alone 4 x e32 of these scenes exceeds 1 (cone_contains 2.1, cone_wide 243: e32.json, "ray_jacobian_plain"); every
# other scene keeps the plain normaliser.
FLOORED_JAC = ("cone_contains", "cone_wide")
FLOOR_BITS = 2.0 ** -20


def scene_tangents(P):
    """{group: [P, c] float32}: randn x VAR_SCALE[group] ** 0.5, fixed seed."""
    g = np.random.RandomState(73)
    return {k: (g.randn(P, ROWS[k].stop - ROWS[k].start) * RFI.VAR_SCALE[k] ** 0.5).astype(np.float32) for k in GROUPS}


def _ordered_sum(a):
    """The sum over axis 1 in ascending index, one rounded addition per column: a pixel's thread."""
    acc = np.zeros(a.shape[0], a.dtype)
    for i in range(a.shape[1]):
        acc = acc + a[:, i]
    return acc


# ------------------------------------------------------------------------------------------------------ the sums
def _pieces(rays, cone, H, W, P, dtype):
    S, Dr = RP.pixel_rays(rays, cone, H, W, dtype)
    step = max(1, PIECE // max(P, 1))
    for view in range(np.asarray(rays).shape[0]):
        for a in range(0, H * W, step):
            s = [S[j][view].reshape(-1, 1)[a:a + step] for j in range(3)]
            d = [Dr[j][view].reshape(-1, 1)[a:a + step] for j in range(3)]
            yield view, slice(a, a + s[0].shape[0]), s, d


def _cloud_cols(xyz, density, scaling, rotation, dtype):
    P = np.asarray(xyz).shape[0]
    return (RP._cols(xyz, dtype), RP._cols(np.asarray(density).reshape(P, 1), dtype)[0], RP._cols(scaling, dtype),
            RP._cols(rotation, dtype))


def jvp_sums(dtype, rays, cone, H, W, xyz, density, scaling, rotation, mod, tan):
    """-> dict(out [V,H,W] in `dtype`, every pair; float64 also N, tail [V,H,W])."""
    f64 = dtype == np.float64
    V, P = np.asarray(rays).shape[0], np.asarray(xyz).shape[0]
    mu, rho, sc, qt = _cloud_cols(xyz, density, scaling, rotation, dtype)
    tn = RFI.stack(tan, dtype)
    res = {k: np.zeros((V, H * W), dtype if k == "out" else np.float64) for k in (("out", "N", "tail") if f64 else ("out",))}
    with np.errstate(all="ignore"):
        for view, idx, s, d in _pieces(rays, cone, H, W, P, dtype):
            o = RP.contract(np, s, d, cone, mu, rho, sc, dtype(mod), qt, None, np.ones_like(s[0]))
            g = o["grads"]
            pair = tn[0][None, :] * g[0]
            for t in range(1, 11):
                pair = pair + tn[t][None, :] * g[t]
            res["out"][view, idx] = pair.sum(1) if f64 else _ordered_sum(pair)
            if f64:
                mag = sum(np.abs(tn[t][None, :] * g[t]) for t in range(11))
                res["N"][view, idx] = mag.sum(1)
                res["tail"][view, idx] = np.where(o["keep"] & (o["q"] > 32.0), mag, 0.0).sum(1)
    return {k: v.reshape(V, H, W) for k, v in res.items()}


def _ray_grad_magnitudes(s, d, mu, rho, scale, mod, quat):
    """gauss_pair_ray_grad's six formulas (csrc/gaussian_ray_grad.hpp) with G = 1 and every addend replaced by its absolute
    value: what g_s and g_d would be if nothing in them cancelled (float64; the pair's quantities are the first lines of
    gaussian_project_ref.contract, as in gaussian_fisher_ref._ray_magnitudes)."""
    a = np.abs
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
    T = a(rho) * t0
    wm = [a(w[i]) + a(k) * a(u[i]) for i in range(3)]   # wp = w - k u, its two addends
    gw = [T * wm[i] for i in range(3)]
    gu = [T * (a(k) * wm[i] + a(u[i]) / A) for i in range(3)]
    ms = [length * (a(M[0][j]) * gw[0] + a(M[1][j]) * gw[1] + a(M[2][j]) * gw[2]) for j in range(3)]
    md = [length * (a(M[0][j]) * gu[0] + a(M[1][j]) * gu[1] + a(M[2][j]) * gu[2]) + (T / length) * a(d[j]) for j in range(3)]
    return ms + md


def jac_sums(dtype, rays, cone, H, W, xyz, density, scaling, rotation, mod):
    """-> dict(out [V,6,H,W] in `dtype`, every pair; float64 also N, tail, M [V,6,H,W]; M: the sum of the pairs' magnitudes)."""
    f64 = dtype == np.float64
    V, P = np.asarray(rays).shape[0], np.asarray(xyz).shape[0]
    mu, rho, sc, qt = _cloud_cols(xyz, density, scaling, rotation, dtype)
    res = {k: np.zeros((V, 6, H * W), dtype if k == "out" else np.float64) for k in (("out", "N", "tail", "M") if f64 else ("out",))}
    with np.errstate(all="ignore"):
        for view, idx, s, d in _pieces(rays, cone, H, W, P, dtype):
            _, gs, gd = RR.pair_ray_grad(s, d, cone, mu, rho, sc, dtype(mod), qt, np.ones_like(s[0]))
            if f64:
                o = RP.contract(np, s, d, cone, mu, rho, sc, dtype(mod), qt)
                far = o["keep"] & (o["q"] > 32.0)
                mags = _ray_grad_magnitudes(s, d, mu, rho, sc, dtype(mod), qt)
            for j, c in enumerate(gs + gd):
                res["out"][view, j, idx] = c.sum(1) if f64 else _ordered_sum(c)
                if f64:
                    res["N"][view, j, idx] = np.abs(c).sum(1)
                    res["tail"][view, j, idx] = np.where(far, np.abs(c), 0.0).sum(1)
                    res["M"][view, j, idx] = np.where(o["keep"], mags[j], 0.0).sum(1)
    return {k: v.reshape(V, 6, H, W) for k, v in res.items()}


def contract_jacobian(jac, rays_tangent, cone):
    """The ray Jacobian [V,6,H,W] contracted with a tangent [V,12] of the rays {a, p00, pu, pv} -> [V,H,W]: the pixel point is
    P = p00 + c pu + r pv; cone beam has ds = t_a, dd = t_P - t_a, parallel beam ds = t_P, dd = t_a.  float64."""
    jac, t = np.asarray(jac, np.float64), np.asarray(rays_tangent, np.float64)
    V, _, H, W = jac.shape
    c, r = np.arange(W)[None, None, :, None], np.arange(H)[None, :, None, None]
    tP = t[:, None, None, 3:6] + c * t[:, None, None, 6:9] + r * t[:, None, None, 9:12]
    ta = np.broadcast_to(t[:, None, None, 0:3], tP.shape)
    ds, dd = (ta, tP - ta) if cone else (tP, ta)
    return sum(jac[:, j] * ds[..., j] + jac[:, 3 + j] * dd[..., j] for j in range(3))


def contract_with_pixel_gradient(jac, G, cone):
    """The ray Jacobian contracted with the pixel gradients G [V,H,W] by pixel_ray_grad's rule and added over the pixels:
    -> dL/drays [V,12], float64."""
    jac, G = np.asarray(jac, np.float64), np.asarray(G, np.float64)
    V, _, H, W = jac.shape
    c, r = np.arange(W)[None, None, :], np.arange(H)[None, :, None]
    out = np.zeros((V, 12))
    for j in range(3):
        gs, gd = G * jac[:, j], G * jac[:, 3 + j]
        gP, ga = (gd, gs - gd) if cone else (gs, gd)
        out[:, j], out[:, 3 + j], out[:, 6 + j], out[:, 9 + j] = ga.sum((1, 2)), gP.sum((1, 2)), (c * gP).sum((1, 2)), (r * gP).sum((1, 2))
    return out


# ------------------------------------------------------------------------------------------------------ references
_CACHE = {}


def reference(name):
    """Float64 sums of a scene, computed once per process: dict(scene, tan, jvp, jac: dicts of out, N, tail)."""
    if name not in _CACHE:
        sc = RFI.proj_scene(name)
        tan = scene_tangents(sc["cloud"][0].shape[0])
        args = (sc["rays"], sc["cone"], sc["H"], sc["W"]) + tuple(sc["cloud"]) + (sc["mod"],)
        jac = jac_sums(np.float64, *args)
        jac["Nplain"] = jac["N"]
        if name in FLOORED_JAC:
            jac["N"] = jac["N"] + FLOOR_BITS * jac["M"]
        _CACHE[name] = {"scene": sc, "tan": tan, "jvp": jvp_sums(np.float64, *args, tan), "jac": jac}
    return _CACHE[name]


def measure_scene_e32(name):
    """-> (e32 of the JVP, e32 of the ray Jacobian, the latter against the plain normaliser): worst |f32 - f64| / normaliser
    over the pixels (and components)."""
    r = reference(name)
    sc = r["scene"]
    args = (sc["rays"], sc["cone"], sc["H"], sc["W"]) + tuple(sc["cloud"]) + (sc["mod"],)
    a = jvp_sums(np.float32, *args, r["tan"])["out"].astype(np.float64)
    b = jac_sums(np.float32, *args)["out"].astype(np.float64)
    return (RP._worst(a - r["jvp"]["out"], r["jvp"]["N"]), RP._worst(b - r["jac"]["out"], r["jac"]["N"]),
            RP._worst(b - r["jac"]["out"], r["jac"]["Nplain"]))


def measure_e32():
    """{"jvp", "ray_jacobian": the e32 the tolerance uses, "ray_jacobian_plain": against sum |g| alone} per scene."""
    out = {"jvp": {}, "ray_jacobian": {}, "ray_jacobian_plain": {}}
    for n in SCENES:
        out["jvp"][n], out["ray_jacobian"][n], out["ray_jacobian_plain"][n] = measure_scene_e32(n)
    return out


def load_e32():
    with open(GOLDEN) as f:
        return json.load(f)


def tolerance(ref, e32):
    """4 x e32 x normaliser + tail + FLOOR, per pixel (and component)."""
    return 4.0 * e32 * ref["N"] + ref["tail"] + FLOOR


def check(got, ref, e32, what):
    """Assert |got - float64| <= tolerance everywhere; prints and returns the worst error in units of the tolerance."""
    got = np.asarray(got, np.float64).reshape(ref["out"].shape)
    tol = tolerance(ref, e32)
    err = np.abs(got - ref["out"])
    worst = float((err / tol).max()) if got.size else 0.0
    print("%s: worst error in units of the tolerance %.3f (<= 1 passes)" % (what, worst))
    bad = ~(err <= tol)
    assert not bad.any(), "%s: %d of %d outside the tolerance, worst %.3g tolerances" % (what, int(bad.sum()), bad.size, worst)
    return worst


# ------------------------------------------------------------------------------------------------------ the geometry LM
# gaussian_project_rays_ref.refine_setup(): cone_p7's geometry, the detector shifted by 1.5 pixels, from offDetector = 0.
LM_ITERS, LM_DAMPING = 3, 1e-3


def lm_solve(A, g, lam):
    """(A + lam diag A) delta = -g, float64."""
    return np.linalg.solve(A + lam * np.diag(np.diag(A)), -g)


def refine_lm_host(setup, dtype, iters=LM_ITERS, damping=LM_DAMPING):
    """refine_geometry_lm's loop on the host: the projection and its ray Jacobian in numpy at `dtype` (float32: the rays are
    rounded to float32 first, as the kernels receive them), d rays / d params by torch in float64, the residual in `dtype` and
    everything after it (the chain rule, the k x k normal equations with Marquardt scaling, the loss) in float64 as in the
    product.  A step is accepted when the mean squared error falls; the damping is divided by 10 then and multiplied by 10
    otherwise.  -> (offDetector [2] float64, loss history [iters]: the loss BEFORE each step, accept sequence)."""
    import torch
    fn = RR.refine_rays_fn(setup)
    H, W = setup["H"], setup["W"]
    target = setup["projs"].astype(dtype)
    cloud = tuple(setup["cloud"])

    def rays_of(p):
        r = fn({"offDetector": torch.from_numpy(p.copy())}).numpy()
        return r.astype(np.float32) if dtype == np.float32 else r

    def residual(p):
        img = jvp_free_image(dtype, rays_of(p), True, H, W, *cloud)
        return (img - target).astype(np.float64)

    p, lam = np.zeros(2), float(damping)
    res = residual(p)
    loss = float((res * res).mean())
    hist, accepts, fresh = [], [], True
    for _ in range(iters):
        hist.append(loss)
        if fresh:
            jac = jac_sums(dtype, rays_of(p), True, H, W, *cloud, 1.0)["out"]
            dr = torch.autograd.functional.jacobian(lambda q: fn({"offDetector": q}), torch.from_numpy(p.copy())).numpy()   # [V,12,2]
            J = np.stack([contract_jacobian(jac, dr[:, :, k], True).reshape(-1) for k in range(p.size)], 1)
            A, g = J.T @ J, J.T @ res.reshape(-1)
        cand = p + lm_solve(A, g, lam)
        rc = residual(cand)
        lc = float((rc * rc).mean())
        fresh = lc < loss
        accepts.append(bool(fresh))
        if fresh:
            p, res, loss, lam = cand, rc, lc, lam / 10.0
        else:
            lam = lam * 10.0
    return p, hist, accepts


def jvp_free_image(dtype, rays, cone, H, W, xyz, density, scaling, rotation, mod=1.0):
    """The projector's image [V,H,W] at `dtype`, every pair (gaussian_project_ref._run without gradients)."""
    return RP._run(dtype, rays, cone, H, W, xyz, density, scaling, rotation, mod)["img"]


def measure_refine_lm():
    st = RR.refine_setup()
    p64, h64, a64 = refine_lm_host(st, np.float64)
    p32, _, a32 = refine_lm_host(st, np.float32)
    true = np.asarray(st["true"])
    return {"iters": LM_ITERS, "damping": LM_DAMPING, "true_offDetector": list(map(float, true)),
            "final64": list(map(float, p64)), "final32": list(map(float, p32)), "f32_minus_f64": float(np.abs(p32 - p64).max()),
            "accepts64": a64, "accepts32": a32, "initial_error64": float(np.abs(true).max()),
            "final_error64": float(np.abs(p64 - true).max()), "loss64": h64}


def load_refine_lm():
    with open(LM_GOLDEN) as f:
        return json.load(f)


# ------------------------------------------------------------------------------------------------------ the cloud's Gauss-Newton
# cone_p7, with xyz, log density, log scaling and rotation perturbed by GN_SIGMA randn(seed GN_SEED) and rounded to float32;
# the target is the float64 projection of the unperturbed cloud rounded to float32.
#
# GN_CG_ITERS.  The 77 x 77 system is badly conditioned (Gaussian 0 is 50 : 1 and thinner than a pixel; near-isotropic
# Gaussians barely feel their quaternion), so a solve carried far amplifies rounding: from 7 CG iterations on the float32 and
# float64 loops drift apart (up to 5 % of the final loss at 10, where the float32 loop rejects a step the float64 loop takes),
# and with dense solves the float64 loop gains a factor 7 in three steps and rejects the third, less than with a truncated
# solve.  A short CG is the regularised solve.  The count is the smallest one (scanned 3 .. 16, float64 and float32) with
# which both loops accept every step -- a rejected last step would leave the last solve untested -- and end below a tenth of
# the initial loss: 3 (a factor 11.1).  Nothing of the product enters this choice.
GN_STEPS, GN_DAMPING, GN_CG_ITERS, GN_SIGMA, GN_SEED, GN_MAX_LOG_STEP = 3, 1e-3, 3, 0.03, 3, 1.0


def gauss_newton_setup():
    sc = RP.scene("cone_p7")
    xyz, dens, scal, rot = (a.astype(np.float64) for a in sc["cloud"])
    g = np.random.RandomState(GN_SEED)
    start = (xyz + GN_SIGMA * g.randn(*xyz.shape), dens * np.exp(GN_SIGMA * g.randn(*dens.shape)),
             scal * np.exp(GN_SIGMA * g.randn(*scal.shape)), rot + GN_SIGMA * g.randn(*rot.shape))
    projs = jvp_free_image(np.float64, sc["rays"], True, sc["H"], sc["W"], *sc["cloud"]).astype(np.float32)
    return {"scene": sc, "rays": sc["rays"], "H": sc["H"], "W": sc["W"], "start": tuple(a.astype(np.float32) for a in start),
            "projs": projs}


def dense_jacobian(dtype, rays, cone, H, W, xyz, density, scaling, rotation, mod=1.0):
    """-> (image [V*H*W], J [V*H*W, 11, P]) at `dtype`: each entry one pair's derivative with G = 1."""
    V, P = np.asarray(rays).shape[0], np.asarray(xyz).shape[0]
    mu, rho, sc, qt = _cloud_cols(xyz, density, scaling, rotation, dtype)
    img, J = np.zeros((V, H * W), dtype), np.zeros((V, H * W, 11, P), dtype)
    with np.errstate(all="ignore"):
        for view, idx, s, d in _pieces(rays, cone, H, W, P, dtype):
            o = RP.contract(np, s, d, cone, mu, rho, sc, dtype(mod), qt, None, np.ones_like(s[0]))
            img[view, idx] = o["term"].sum(1) if dtype == np.float64 else _ordered_sum(o["term"])
            for t in range(11):
                J[view, idx, t] = o["grads"][t]
    return img.reshape(-1), J.reshape(V * H * W, 11, P)


def log_factors(cloud, log_density=True, log_scaling=True):
    """[11, P] float64: what a tangent in the solver's variables is multiplied by to become one in the kernels' parameters --
    the density for log density, the scales for log scales, 1 elsewhere."""
    xyz, dens, scal, rot = (np.asarray(a, np.float64) for a in cloud)
    P = xyz.shape[0]
    f = np.ones((11, P))
    if log_density:
        f[3] = dens.reshape(-1)
    if log_scaling:
        f[4:7] = scal.T
    return f


def cg_solve(matvec, b, minv, iters):
    """`iters` steps of preconditioned conjugate gradients on matvec(x) = b from x = 0, float64 scalars; a step whose curvature
    is not positive changes nothing."""
    x = np.zeros_like(b)
    r = b.copy()
    z = minv * r
    p = z.copy()
    rz = float((r.astype(np.float64) * z).sum())
    for _ in range(iters):
        Ap = matvec(p)
        pAp = float((p.astype(np.float64) * Ap).sum())
        alpha = rz / pAp if pAp > 0 else 0.0
        x = x + (alpha * p).astype(b.dtype)
        r = r - (alpha * Ap).astype(b.dtype)
        z = minv * r
        rz_new = float((r.astype(np.float64) * z).sum())
        beta = rz_new / rz if rz > 0 else 0.0
        p = z + (beta * p).astype(b.dtype)
        rz = rz_new
    return x


def apply_step(cloud, delta, log_density=True, log_scaling=True, max_log_step=1.0):
    """cloud (float32 arrays) moved by delta [11, P] in the solver's variables, rounded to float32; a step in a log variable
    is clipped to +- max_log_step (gauss_newton_step's argument: an unclipped one can underflow exp to 0 in float32)."""
    xyz, dens, scal, rot = (np.asarray(a, np.float32) for a in cloud)
    d = np.asarray(delta, np.float32)
    dd, ds = d[3].reshape(dens.shape), d[4:7].T
    if log_density:
        dd = np.clip(dd, -max_log_step, max_log_step)
    if log_scaling:
        ds = np.clip(ds, -max_log_step, max_log_step)
    with np.errstate(over="ignore"):   # a wild candidate is the LM rule's to reject
        return _moved(xyz, dens, scal, rot, d, dd, ds, log_density, log_scaling)


def _moved(xyz, dens, scal, rot, d, dd, ds, log_density, log_scaling):
    return (xyz + d[0:3].T, dens * np.exp(dd) if log_density else dens + dd, scal * np.exp(ds) if log_scaling else scal + ds,
            rot + d[7:11].T)


def _jt(J, g):
    """J^T g by numpy's own sums (no BLAS: the same bits wherever numpy is the same)."""
    return (J * g[:, None]).sum(0)


def refine_cloud_host(setup, dtype, steps=GN_STEPS, cg_iters=GN_CG_ITERS, damping=GN_DAMPING, max_log_step=GN_MAX_LOG_STEP):
    """refine_cloud's loop on the host with a dense J at `dtype`: per step the image and J at the current cloud, F = diag J^T J,
    cg_iters steps of Jacobi-preconditioned CG on (J^T J + lam diag F) delta = -J^T r in the log variables (cg_iters = None:
    a dense least-squares solve), the candidate's loss, and the LM rule of the geometry loop.  J t and J^T g are summed at `dtype`, the CG
    vectors are held at `dtype`, its scalars and the loss in float64.  -> (cloud, loss history [steps + 1]: the loss before each step and the final one, accept sequence, the candidates' losses)."""
    rays, H, W = setup["rays"], setup["H"], setup["W"]
    target = setup["projs"].astype(dtype)
    cloud, lam = tuple(setup["start"]), float(damping)
    hist, accepts, tried = [], [], []

    def loss_of(c):
        img = jvp_free_image(dtype, rays, True, H, W, *c).reshape(-1)
        r = img - target.reshape(-1)
        return float((r.astype(np.float64) ** 2).mean()), r

    loss, res = loss_of(cloud)
    fresh = True
    for _ in range(steps):
        hist.append(loss)
        if fresh:
            _, J = dense_jacobian(dtype, rays, True, H, W, *cloud)
            f = log_factors(cloud).astype(dtype)
            J = (J * f[None]).reshape(J.shape[0], -1)
            F = (J * J).sum(0)
            b = -_jt(J, res)
        if cg_iters is None:
            delta = np.linalg.lstsq((J.T @ J + lam * np.diag(F)).astype(np.float64), b.astype(np.float64), rcond=None)[0]
        else:
            M = (1.0 + lam) * F.astype(np.float64)
            minv = np.where(M > 0, 1.0 / np.where(M > 0, M, 1.0), 0.0).astype(dtype)
            delta = cg_solve(lambda t: _jt(J, (J * t[None, :]).sum(1)) + dtype(lam) * F * t, b, minv, cg_iters)
        cand = apply_step(cloud, np.asarray(delta).reshape(11, -1), max_log_step=max_log_step)
        lc, rc = loss_of(cand)
        tried.append(lc)
        fresh = lc < loss
        accepts.append(bool(fresh))
        if fresh:
            cloud, loss, res, lam = cand, lc, rc, lam / 10.0
        else:
            lam = lam * 10.0
    final, _ = loss_of(cloud)
    return cloud, hist + [final], accepts, tried


def measure_gauss_newton():
    st = gauss_newton_setup()
    _, h64, a64, t64 = refine_cloud_host(st, np.float64)
    _, h32, a32, _ = refine_cloud_host(st, np.float32)
    _, hex64, _, _ = refine_cloud_host(st, np.float64, cg_iters=None)
    return {"steps": GN_STEPS, "damping": GN_DAMPING, "cg_iters": GN_CG_ITERS, "sigma": GN_SIGMA, "seed": GN_SEED,
            "max_log_step": GN_MAX_LOG_STEP, "gain64": h64[0] / h64[-1], "gain32": h32[0] / h32[-1],
            "loss64": h64, "loss32": h32, "loss64_exact_solves": hex64, "accepts64": a64, "accepts32": a32,
            "candidates64": t64, "f32_minus_f64": abs(h32[-1] - h64[-1])}


def load_gauss_newton():
    with open(GN_GOLDEN) as f:
        return json.load(f)


if __name__ == "__main__":
    os.makedirs(GOLDEN_DIR, exist_ok=True)
    res = measure_e32()
    with open(GOLDEN, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    for n in SCENES:
        print(n, "jvp %.3e  ray jacobian %.3e" % (res["jvp"][n], res["ray_jacobian"][n]))
    for path, m in ((LM_GOLDEN, measure_refine_lm()), (GN_GOLDEN, measure_gauss_newton())):
        with open(path, "w") as f:
            json.dump(m, f, indent=1, sort_keys=True)
        print(m)
