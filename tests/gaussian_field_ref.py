"""Restatement of the exact field query's contract (include/r2hip.h: r2_query_gaussians and its backward;
csrc/gaussian_points.hpp), the scenes its tests share, and the measured float32 error the GPU tolerance is taken from.  Host
only; the product never imports this file.  It mirrors tests/gaussian_project_ref.py and takes quat_to_rot's entries, the
cloud generator and the underflow floor from it.

One body of arithmetic, ``contract``, written component by component in the operation order of gaussian_points.hpp (which
hands the pair to gaussian_rays.hpp's gradient with u = 0 and |d| = 1: the terms that vanish there are left out here, they
are exact zeros) with nothing but + - * / exp, runs on numpy or torch arrays of any float dtype:

* numpy float64 is the reference (``field64``); ``qmax`` cuts the sum at q <= qmax and ``tmin`` at term >= tmin, None sums
  every pair;
* torch float64 is the same body under autograd (``torch_field``), for the gradcheck of the analytic gradients;
* numpy float32 is the float32 restatement in the contract's operation order (``field32``): each numpy operation rounds once,
  as each operation of the kernels does (they are built without FMA contraction).

``measure_e32`` is that error per scene: for the values the worst |f32 - f64| / sum_g |term_g| over the points, for each of
the five gradients the worst |f32 - f64| / sum_pairs |contribution| over its components (denominators under FLOOR are left
out and checked absolutely instead).  tests/golden/gaussian_field/e32.json holds it (written by
``python -m tests.gaussian_field_ref``); the GPU tests allow 4 x that.
"""
import json
import math
import os

import numpy as np

from tests.gaussian_project_ref import FLOOR, _cloud, _cols, _rot, _worst

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gaussian_field", "e32.json")
GRADS = ("xyz", "density", "scaling", "rotation", "points")
SPHERE = math.sqrt(32.0) * 1.01


# ------------------------------------------------------------------------------------------------------ the contract
def contract(xp, x, mu, rho, scale, mod, quat, qmax=None, tmin=None, G=None):
    """All pairs of N points and P Gaussians.  x: three [N,1] arrays; mu, scale: three [1,P] arrays; rho: [1,P]; quat: four
    [1,P]; G: [N,1] or None.  -> dict(term [N,P], keep [N,P] bool, q [N,P], and with G: grads: fourteen [N,P] arrays, d mu
    (3), d rho, d scale (3), d quaternion (4), d x (3))."""
    R = _rot(quat)
    isg = [1.0 / (scale[i] * mod) for i in range(3)]
    M = [[R[j][i] * isg[i] for j in range(3)] for i in range(3)]
    e = [x[j] - mu[j] for j in range(3)]
    w = [M[i][0] * e[0] + M[i][1] * e[1] + M[i][2] * e[2] for i in range(3)]
    q = w[0] * w[0] + w[1] * w[1] + w[2] * w[2]
    ex = xp.exp(-0.5 * q)
    term = rho * (ex * 1.0)
    # gauss_radius' rule (a non-finite parameter or a scale <= 0: nothing), a finite point, a finite q
    allp = mu[0] + mu[1] + mu[2] + rho + scale[0] + scale[1] + scale[2] + quat[0] + quat[1] + quat[2] + quat[3]
    keep = (xp.abs(allp) < math.inf) & (scale[0] * mod > 0) & (scale[1] * mod > 0) & (scale[2] * mod > 0)
    keep = keep & (xp.abs(x[0]) < math.inf) & (xp.abs(x[1]) < math.inf) & (xp.abs(x[2]) < math.inf) & (q < math.inf)
    if qmax is not None:
        keep = keep & (q <= qmax)
    if tmin is not None:
        keep = keep & (term >= tmin)
    out = {"term": xp.where(keep, term, xp.zeros_like(term)), "keep": keep, "q": q, "e": e}
    if G is None:
        return out
    T = rho * ex
    gw = [-(T * w[i]) for i in range(3)]
    hw = [gw[i] * isg[i] for i in range(3)]
    o = [-(G * (M[0][j] * gw[0] + M[1][j] * gw[1] + M[2][j] * gw[2])) for j in range(3)]
    o.append(G * (ex * 1.0))
    o += [-(G * ((gw[i] * w[i]) / scale[i])) for i in range(3)]
    D = [[G * (e[j] * hw[i]) for i in range(3)] for j in range(3)]
    r, qx, y, z = quat
    o.append(2.0 * (z * (D[1][0] - D[0][1]) + y * (D[0][2] - D[2][0]) + qx * (D[2][1] - D[1][2])))
    o.append(2.0 * (y * (D[0][1] + D[1][0]) + z * (D[0][2] + D[2][0]) + r * (D[2][1] - D[1][2])) - 4.0 * (qx * (D[1][1] + D[2][2])))
    o.append(2.0 * (qx * (D[0][1] + D[1][0]) + r * (D[0][2] - D[2][0]) + z * (D[1][2] + D[2][1])) - 4.0 * (y * (D[0][0] + D[2][2])))
    o.append(2.0 * (r * (D[1][0] - D[0][1]) + qx * (D[0][2] + D[2][0]) + y * (D[1][2] + D[2][1])) - 4.0 * (z * (D[0][0] + D[1][1])))
    o += [-o[j] for j in range(3)]
    out["grads"] = [xp.where(keep, c, xp.zeros_like(c)) for c in o]
    return out


def _split(a, b):
    return {"xyz": a[0:3].T.copy(), "density": a[3:4].T.copy(), "scaling": a[4:7].T.copy(), "rotation": a[7:11].T.copy(),
            "points": b.copy()}


def _run(dtype, points, xyz, density, scaling, rotation, mod=1.0, qmax=None, tmin=None, G=None):
    """-> dict(val [N], abs [N] = sum_g |term_g|, and with G [N]: grads {name: array}, gabs {name: array})."""
    pts = np.asarray(points, np.float32).reshape(-1, 3).astype(dtype)
    N, P = pts.shape[0], np.asarray(xyz).shape[0]
    cols = lambda a, c: _cols(np.asarray(a, np.float32).reshape(P, c), dtype) if P else [np.zeros((1, 0), dtype)] * c
    mu, sc, qt, rho = cols(xyz, 3), cols(scaling, 3), cols(rotation, 4), cols(density, 1)[0]
    mod = dtype(mod)
    val, ab = np.zeros(N, dtype), np.zeros(N, dtype)
    gsum, gabs = np.zeros((11, P), dtype), np.zeros((11, P), dtype)
    psum, pabs = np.zeros((N, 3), dtype), np.zeros((N, 3), dtype)
    step = max(1, (1 << 21) // max(P, 1))   # points per piece (memory)
    with np.errstate(all="ignore"):
        for a in range(0, N, step):
            x = [pts[a:a + step, j:j + 1] for j in range(3)]
            Gv = None if G is None else np.asarray(G, np.float32).astype(dtype).reshape(-1, 1)[a:a + step]
            o = contract(np, x, mu, rho, sc, mod, qt, qmax, tmin, Gv)
            if P:
                val[a:a + step] = o["term"].sum(1)
                ab[a:a + step] = np.abs(o["term"]).sum(1)
            if G is not None:
                for t, c in enumerate(o["grads"][:11]):
                    gsum[t] += c.sum(0)
                    gabs[t] += np.abs(c).sum(0)
                for j, c in enumerate(o["grads"][11:]):
                    psum[a:a + step, j] = c.sum(1)
                    pabs[a:a + step, j] = np.abs(c).sum(1)
    out = {"val": val, "abs": ab}
    if G is not None:
        out["grads"], out["gabs"] = _split(gsum, psum), _split(gabs, pabs)
    return out


def field64(points, xyz, density, scaling, rotation, mod=1.0, qmax=None, tmin=None, G=None):
    return _run(np.float64, points, xyz, density, scaling, rotation, mod, qmax, tmin, G)


def field32(points, xyz, density, scaling, rotation, mod=1.0, G=None):
    return _run(np.float32, points, xyz, density, scaling, rotation, mod, None, None, G)


def torch_field(points, xyz, density, scaling, rotation, mod=1.0):
    """The same body on torch float64 tensors, differentiable in all five: -> [N]."""
    import torch
    cols = lambda t: [t[:, j][None, :] for j in range(t.shape[1])]
    x = [points[:, j][:, None] for j in range(3)]
    return contract(torch, x, cols(xyz), density.reshape(1, -1), cols(scaling), mod, cols(rotation))["term"].sum(1)


def sphere_radius(scaling, rotation, mod=1.0):
    """gauss_radius (csrc/gaussian_rays.hpp) in float64: [P]; inf where R is (nearly) singular."""
    s = np.asarray(scaling, np.float64) * mod
    q = np.asarray(rotation, np.float64)
    n2 = (q * q).sum(1)
    om = 1.0 - n2
    smin2 = np.minimum(1.0, om * om + 2.0 * om * (2.0 * q[:, 0] ** 2 - n2) + n2 * n2)
    with np.errstate(all="ignore"):
        return np.where(smin2 > 1e-6, SPHERE * s.max(1) / np.sqrt(np.maximum(smin2, 1e-300)), np.inf)


# ------------------------------------------------------------------------------------------------------ the shared scenes
PLANE = {"origin": (-0.5, -0.4, -0.3), "du": (0.04, 0.01, 0.012), "dv": (-0.008, 0.045, 0.02), "H": 24, "W": 20}
PATCH = {"center": (0.1, -0.05, 0.0), "nVoxel": (12, 12, 12), "sVoxel": (0.3, 0.3, 0.3)}
TAILS = (1, 255, 256, 257, 513)


def plane_lattice(origin, du, dv, H, W):
    """field.plane_points in numpy float32: [H,W,3]."""
    o, u, v = (np.asarray(a, np.float32) for a in (origin, du, dv))
    c = np.arange(W, dtype=np.float32)[None, :, None]
    r = np.arange(H, dtype=np.float32)[:, None, None]
    return ((o + c * u) + r * v).astype(np.float32)


def patch_centres(center, nVoxel, sVoxel):
    """field.voxel_centres in numpy: [nx,ny,nz,3] float32."""
    ax = [float(c) - float(s) / 2 + (np.arange(int(n), dtype=np.float64) + 0.5) * (float(s) / int(n))
          for c, n, s in zip(center, nVoxel, sVoxel)]
    return np.stack(np.meshgrid(*ax, indexing="ij"), -1).astype(np.float32)


def _uniform(N, seed, half=0.6):
    return ((np.random.RandomState(seed).rand(N, 3) * 2 - 1) * half).astype(np.float32)


def scene(name):
    """-> dict(points [..., 3] float32, cloud = (xyz, density, scaling, rotation) float32 arrays, mod, G [N] float32;
    zero_gaussians / zero_points: indices that must contribute / receive exact zeros)."""
    mod, zg, zp = 1.0, [], []
    if name == "plane":
        cloud, pts = _cloud(300, 401), plane_lattice(**PLANE)
    elif name == "patch":
        cloud, pts = _cloud(300, 401), patch_centres(**PATCH)
    elif name == "scattered":
        cloud, pts = _cloud(300, 401), _uniform(777, 12)
    elif name.startswith("tail_"):
        cloud, pts = _cloud(40, 402, lo=0.03, hi=0.3), _uniform(int(name[5:]), 13)
    elif name == "many":
        cloud, pts = _cloud(700, 403), _uniform(300, 14)
    elif name == "none":
        cloud, pts = tuple(np.zeros((0, c), np.float32) for c in (3, 1, 3, 4)), _uniform(100, 15)
    elif name == "far":   # spheres of at most 5.72 * 0.03 around means within 0.3 of the origin; points at least 2.4 away
        cloud, pts = _cloud(50, 404, lo=0.01, hi=0.03, spread=0.3), _uniform(300, 16)
        pts[:, 0] += np.where(pts[:, 0] >= 0, 3.0, -3.0).astype(np.float32)
    elif name == "offset":   # cloud and points moved by 100 x the extent: x - mu cancels seven digits
        cloud, pts = _cloud(50, 405, lo=0.05, hi=0.3), _uniform(200, 17)
        shift = np.array([100.0, -100.0, 100.0], np.float32)
        cloud, pts = (cloud[0] + shift,) + cloud[1:], pts + shift
    elif name == "tiny":     # sigma = 5e-4 on every axis, points within a few sigma of a mean
        xyz, dens, sc, q = _cloud(20, 406, spread=0.01)
        sc = np.full_like(sc, 5e-4)
        g = np.random.RandomState(18)
        pts = (xyz[np.arange(200) % 20] + g.randn(200, 3) * 1.5 * 5e-4).astype(np.float32)
        cloud = (xyz, dens, sc, q)
    elif name == "bad":
        xyz, dens, sc, q = (a.copy() for a in _cloud(12, 407, lo=0.05, hi=0.3))
        xyz[1, 2], sc[2, 0], sc[3, 1] = np.nan, np.inf, 0.0
        pts = _uniform(64, 19)
        pts[5, 1], pts[9, 0] = np.nan, np.inf
        cloud, zg, zp = (xyz, dens, sc, q), [1, 2, 3], [5, 9]
    elif name == "raw_quat":   # quaternions used as they come: norms 0.3 .. 3
        xyz, dens, sc, q = _cloud(60, 408, lo=0.03, hi=0.3)
        q = (q * np.exp(np.random.RandomState(20).uniform(np.log(0.3), np.log(3.0), (60, 1)))).astype(np.float32)
        cloud, pts = (xyz, dens, sc, q), _uniform(200, 21)
    elif name in ("mod_half", "mod_two"):
        cloud, pts, mod = _cloud(60, 409, lo=0.03, hi=0.3), _uniform(200, 22), {"mod_half": 0.5, "mod_two": 2.0}[name]
    else:
        raise KeyError(name)
    N = pts.reshape(-1, 3).shape[0]
    G = (np.random.RandomState(5).rand(N) * 2 - 1).astype(np.float32)
    return {"points": np.ascontiguousarray(pts, np.float32), "cloud": cloud, "mod": mod, "G": G, "zero_gaussians": zg,
            "zero_points": zp}


SCENES = ("plane", "patch", "scattered") + tuple("tail_%d" % n for n in TAILS) + (
    "many", "none", "far", "offset", "tiny", "bad", "raw_quat", "mod_half", "mod_two")

_CACHE = {}


def reference(name):
    """Float64 results of a scene, computed once per process: dict(scene, lo, hi: field64 with qmax = 32 and None, with G)."""
    if name not in _CACHE:
        sc = scene(name)
        _CACHE[name] = {"scene": sc, "lo": field64(sc["points"], *sc["cloud"], mod=sc["mod"], qmax=32.0, G=sc["G"]),
                        "hi": field64(sc["points"], *sc["cloud"], mod=sc["mod"], G=sc["G"])}
    return _CACHE[name]


VOXEL_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "voxel_tv_150_16x16x16.npz")


def voxel_bracket():
    """The 16^3 grid of 150 Gaussians of tests/golden/voxel_tv_150_16x16x16.npz (unit quaternions, scale_modifier 1) and the
    bracket the voxelizer's volume of it must lie in at every voxel: -> dict(cloud, nVoxel, sVoxel, center, lo, hi [16,16,16]).

    Upper limit: the field itself, every pair.  Lower limit: the pairs with q <= 9 and term >= 2e-6.  The voxelizer sums a
    pair when the voxel lies in a tile that the cube of rad = ceil(3 max(scale) / dVoxel) voxels around the mean touches and
    alpha = rho exp(power) >= 1e-6.  q <= 9 puts the voxel centre within 3 sigma_max <= rad dVoxel of the mean on every axis,
    inside the cube; term >= 2e-6 keeps alpha above the cut whatever float32 does to it (a factor 2 where 1e-5 would do).
    Each limit is widened by the 1e-4 sum |terms| the project claims for volumes."""
    if "voxel" not in _CACHE:
        d = np.load(VOXEL_GOLDEN)
        assert float(d["in_params"][0]) == 1.0
        cloud = tuple(d[k].astype(np.float32) for k in ("in_means3D", "in_opacities", "in_scales", "in_rotations"))
        geo = {"center": tuple(float(v) for v in d["in_center"]), "nVoxel": tuple(int(v) for v in d["in_nVoxel"]),
               "sVoxel": tuple(float(v) for v in d["in_sVoxel"])}
        pts = patch_centres(**geo)
        lower, upper = field64(pts, *cloud, qmax=9.0, tmin=2e-6), field64(pts, *cloud)
        shape = geo["nVoxel"]
        _CACHE["voxel"] = dict(geo, cloud=cloud, lo=(lower["val"] - 1e-4 * lower["abs"]).reshape(shape),
                               hi=(upper["val"] + 1e-4 * upper["abs"]).reshape(shape))
    return _CACHE["voxel"]


def error_against(ref, got_val, got_grads=None):
    """Worst normalised error of values (and gradients) against a float64 result `ref` of field64(..., G=...)."""
    out = {"value": _worst(np.asarray(got_val, np.float64).reshape(-1) - ref["val"], ref["abs"])}
    if got_grads is not None:
        for k in GRADS:
            out[k] = _worst(np.asarray(got_grads[k], np.float64).reshape(ref["grads"][k].shape) - ref["grads"][k], ref["gabs"][k])
    return out


def measure_e32(name):
    r = reference(name)
    sc = r["scene"]
    f32 = field32(sc["points"], *sc["cloud"], mod=sc["mod"], G=sc["G"])
    return error_against(r["hi"], f32["val"], f32["grads"])


def load_e32():
    with open(GOLDEN) as f:
        return json.load(f)


if __name__ == "__main__":
    os.makedirs(os.path.dirname(GOLDEN), exist_ok=True)
    res = {n: measure_e32(n) for n in SCENES}
    with open(GOLDEN, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    for n, v in res.items():
        print(n, " ".join("%s %.3e" % kv for kv in v.items()))
