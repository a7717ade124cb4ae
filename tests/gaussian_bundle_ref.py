"""Restatement of the contract of the exact line integrals along caller-supplied rays (include/r2hip.h:
r2_integrate_gaussians and its backward; csrc/gaussian_bundle.hpp), the scenes its tests share, and the measured float32
error the GPU tolerance is taken from.  Host only; the product never imports this file.  It mirrors
tests/gaussian_field_ref.py.

The pair and its eleven parameter gradients are tests/gaussian_project_ref.py's ``contract`` and the two ray gradients
tests/gaussian_project_rays_ref.py's ``pair_ray_grad``, imported, not copied; what is added here is what the bundle's contract
adds: which rays are valid (six finite numbers and a float32 length that is positive and finite), which Gaussians are
(gauss_radius' rule: finite parameters, every scale_modifier * scale > 0), and the sums per ray and per Gaussian.

* numpy float64 is the reference (``bundle64``); ``qmax`` cuts the sums at q <= qmax, None sums every pair;
* torch float64 is the pair under autograd (``torch_bundle``), for the check of the analytic gradients;
* numpy float32 is the float32 restatement in the contract's operation order (``bundle32``): each numpy operation rounds once,
  as each operation of the kernels does (they are built without FMA contraction).

``measure_e32`` is that error per scene: for the values the worst |f32 - f64| / sum_g |term_g| over the rays, for each of the
six gradient groups the worst |f32 - f64| / sum_pairs |contribution| over its components (denominators under FLOOR are left
out and checked absolutely instead).  tests/golden/gaussian_bundle/e32.json holds it (written by
``python -m tests.gaussian_bundle_ref``); the GPU tests allow 4 x that.
"""
import json
import os

import numpy as np

from tests import gaussian_project_rays_ref as RR
from tests import gaussian_project_ref as R
from tests.gaussian_project_ref import FLOOR, _cloud, _cols, _worst

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gaussian_bundle", "e32.json")
PARAMS = ("xyz", "density", "scaling", "rotation")
GRADS = PARAMS + ("origins", "directions")


# ------------------------------------------------------------------------------------------------------ the contract
def valid_rays(origins, directions):
    """[N] bool, decided in float32 as the kernels decide it."""
    o, d = np.asarray(origins, np.float32).reshape(-1, 3), np.asarray(directions, np.float32).reshape(-1, 3)
    with np.errstate(all="ignore"):
        length = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])
        return np.isfinite(o).all(1) & np.isfinite(d).all(1) & (length > 0) & np.isfinite(length)


def valid_gaussians(xyz, density, scaling, rotation, mod):
    """[P] bool: gauss_radius >= 0 (csrc/gaussian_rays.hpp)."""
    P = np.asarray(xyz).shape[0]
    a = np.concatenate([np.asarray(t, np.float32).reshape(P, -1) for t in (xyz, density, scaling, rotation)], 1)
    with np.errstate(all="ignore"):
        s = np.asarray(scaling, np.float32).reshape(P, 3) * np.float32(mod)
        return np.isfinite(a.sum(1) + np.float32(mod)) & (s > 0).all(1)


def _split(a, gs, gd):
    return {"xyz": a[0:3].T.copy(), "density": a[3:4].T.copy(), "scaling": a[4:7].T.copy(), "rotation": a[7:11].T.copy(),
            "origins": gs.copy(), "directions": gd.copy()}


def _run(dtype, origins, directions, half_line, xyz, density, scaling, rotation, mod=1.0, qmax=None, G=None):
    """-> dict(val [N], abs [N] = sum_g |term_g|, and with G [N]: grads {name: array}, gabs {name: array}).  The rays are
    cast to `dtype` as they come (float32 rays are exact in both; float64 rays stay float64 in a float64 run)."""
    o32, d32 = np.asarray(origins, np.float32).reshape(-1, 3), np.asarray(directions, np.float32).reshape(-1, 3)
    N, P = o32.shape[0], np.asarray(xyz).shape[0]
    cols = lambda a, c: _cols(np.asarray(a, np.float32).reshape(P, c), dtype) if P else [np.zeros((1, 0), dtype)] * c
    mu, sc, qt, rho = cols(xyz, 3), cols(scaling, 3), cols(rotation, 4), cols(density, 1)[0]
    ok = valid_rays(o32, d32)[:, None] & (valid_gaussians(xyz, density, scaling, rotation, mod)[None, :] if P else np.zeros((1, 0), bool))
    o, d = np.asarray(origins).reshape(-1, 3).astype(dtype), np.asarray(directions).reshape(-1, 3).astype(dtype)
    mod = dtype(mod)
    val, ab = np.zeros(N, dtype), np.zeros(N, dtype)
    gsum, gabs = np.zeros((11, P), dtype), np.zeros((11, P), dtype)
    rsum, rabs = np.zeros((2, N, 3), dtype), np.zeros((2, N, 3), dtype)
    step = max(1, (1 << 20) // max(P, 1))   # rays per piece (memory)
    with np.errstate(all="ignore"):
        for a in range(0, N if P else 0, step):
            s = [o[a:a + step, j:j + 1] for j in range(3)]
            dd = [d[a:a + step, j:j + 1] for j in range(3)]
            m = ok[a:a + step]
            zero = lambda c: np.where(m, c, np.zeros_like(c))
            Gv = None if G is None else np.asarray(G, np.float32).astype(dtype).reshape(-1, 1)[a:a + step]
            c = R.contract(np, s, dd, half_line, mu, rho, sc, mod, qt, qmax, Gv)
            term = zero(c["term"])
            val[a:a + step] = term.sum(1)
            ab[a:a + step] = np.abs(term).sum(1)
            if G is None:
                continue
            for t, g in enumerate(c["grads"]):
                g = zero(g)
                gsum[t] += g.sum(0)
                gabs[t] += np.abs(g).sum(0)
            _, gs, gd = RR.pair_ray_grad(s, dd, half_line, mu, rho, sc, mod, qt, Gv, qmax)
            for w, grp in enumerate((gs, gd)):
                for j in range(3):
                    g = zero(grp[j])
                    rsum[w, a:a + step, j] = g.sum(1)
                    rabs[w, a:a + step, j] = np.abs(g).sum(1)
    out = {"val": val, "abs": ab}
    if G is not None:
        out["grads"], out["gabs"] = _split(gsum, rsum[0], rsum[1]), _split(gabs, rabs[0], rabs[1])
    return out


def bundle64(origins, directions, half_line, xyz, density, scaling, rotation, mod=1.0, qmax=None, G=None):
    return _run(np.float64, origins, directions, half_line, xyz, density, scaling, rotation, mod, qmax, G)


def bundle32(origins, directions, half_line, xyz, density, scaling, rotation, mod=1.0, G=None):
    return _run(np.float32, origins, directions, half_line, xyz, density, scaling, rotation, mod, None, G)


def torch_bundle(origins, directions, half_line, xyz, density, scaling, rotation, mod=1.0):
    """The pair on torch float64 tensors, differentiable in all six: -> [N].  For valid rays and Gaussians."""
    cols = lambda t: [t[:, j][None, :] for j in range(t.shape[1])]
    s = [origins[:, j][:, None] for j in range(3)]
    d = [directions[:, j][:, None] for j in range(3)]
    import torch
    return R.contract(torch, s, d, half_line, cols(xyz), density.reshape(1, -1), cols(scaling), mod, cols(rotation))["term"].sum(1)


# ------------------------------------------------------------------------------------------------------ the shared scenes
TAILS = (1, 255, 256, 257, 513)
CURVED = {"angles": (0.3, 2.4), "DSO": 5.0, "DSD": 7.0, "dGamma": 0.012, "dV": 0.09, "nDetector": (9, 31), "offDetector": (0.02, -0.05)}


def _lines(N, seed, half=0.5, reach=4.0, lo=0.01, hi=100.0, past=0.25):
    """N random lines: through a point uniform in the cube of half-side `half` (a fraction `past` of them through one three
    times as far out: past the cloud), in a uniform direction of length log-uniform in [lo, hi], the start moved back along
    the line by up to `reach`."""
    g = np.random.RandomState(seed)
    through = (g.rand(N, 3) * 2 - 1) * half
    through[g.rand(N) < past] *= 3.0
    d = g.randn(N, 3)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    start = through - d * (g.rand(N, 1) * reach)
    d *= np.exp(g.uniform(np.log(lo), np.log(hi), (N, 1)))
    return start.astype(np.float32), d.astype(np.float32)


def flat_rays(beam):
    """The [V,12] rays, the detector and the cloud of gaussian_project_ref's 17 x 23 scene with 300 Gaussians, and its pixel
    rays through geometry.pixel_rays (float32, as the projector forms them)."""
    import torch
    from r2_gaussian_amd import geometry
    sc = R.scene(beam + "_p300_small")
    o, d = geometry.pixel_rays(torch.from_numpy(sc["rays"]), sc["cone"], sc["H"], sc["W"])
    return sc, o.contiguous().numpy(), d.contiguous().numpy()


def scene(name):
    """-> dict(origins, directions [..., 3] float32, half_line, cloud = (xyz, density, scaling, rotation) float32 arrays, mod,
    G [N] float32; zero_gaussians / zero_rays: indices that must contribute / receive exact zeros)."""
    mod, half, zg, zr = 1.0, False, [], []
    if name in ("flat_cone", "flat_parallel"):
        sc, o, d = flat_rays(name[5:])
        cloud, half = sc["cloud"], sc["cone"]
    elif name == "scattered":
        cloud, (o, d) = _cloud(300, 501), _lines(777, 31)
    elif name.startswith("tail_"):
        cloud, (o, d) = _cloud(40, 502, lo=0.03, hi=0.3), _lines(int(name[5:]), 32)
    elif name == "many":   # two full rounds of 256 Gaussians and a partial one
        cloud, (o, d) = _cloud(700, 503), _lines(300, 33)
    elif name == "none":
        cloud, (o, d) = tuple(np.zeros((0, c), np.float32) for c in (3, 1, 3, 4)), _lines(100, 34)
    elif name == "curved":
        import torch
        from r2_gaussian_amd import geometry
        o, d = (t.numpy().astype(np.float32) for t in geometry.curved_detector_rays(torch.tensor(CURVED["angles"], dtype=torch.float64),
                                                                                   **{k: v for k, v in CURVED.items() if k != "angles"}))
        cloud, half = _cloud(300, 504), True
    elif name == "miss":   # spheres within 0.5 of the origin; lines at |x| >= 2.4 that come no closer than 190 along y, z
        cloud = _cloud(50, 505, lo=0.01, hi=0.03, spread=0.3)
        g = np.random.RandomState(35)
        o = ((g.rand(300, 3) * 2 - 1) * 0.6).astype(np.float32)
        o[:, 0] += np.where(o[:, 0] >= 0, 3.0, -3.0).astype(np.float32)
        d = g.randn(300, 3)
        d[:, 0] = np.where(np.arange(300) % 2 == 0, 0.0, 0.01 * g.uniform(-1, 1, 300) * np.linalg.norm(d[:, 1:], axis=1))
        d = (d * np.exp(g.uniform(np.log(0.01), np.log(100.0), (300, 1)))).astype(np.float32)
    elif name == "inside":   # half lines that start inside the cloud: the cone rule decides about half of the pairs
        cloud, (o, d), half = _cloud(300, 506), _lines(300, 36, half=0.4, reach=0.0, past=0.0), True
    elif name in ("offset", "offset_tiny"):   # cloud and rays moved by 100 x the extent
        shift = np.array([100.0, -100.0, 100.0], np.float32)
        if name == "offset":
            cloud, (o, d) = _cloud(50, 507, lo=0.05, hi=0.3), _lines(200, 37)
        else:
            sc = scene("tiny")
            cloud, o, d = sc["cloud"], sc["origins"], sc["directions"]
        cloud, o = (cloud[0] + shift,) + cloud[1:], o + shift
    elif name == "tiny":   # sigma = 5e-4, the starts six units away, the lines within a few sigma of a mean
        # The three scales of a Gaussian lie within a factor 1.25 either side of 5e-4 (as gaussian_project_ref's small_sigma
        # scene has them around 0.01), not at 5e-4 exactly: with three equal scales the rotation gradient is analytically zero
        # for a unit quaternion, its float64 value and sum of |contributions| are what the float32 rounding of the quaternion's
        # norm leaves, and the check would hold rounding noise against rounding noise -- on the host, moving exp by one unit in
        # the last place (which the device's expf is free to do) moves the float32 restatement's rotation error of that scene
        # by up to 7.1 x its e32, of this one by up to 2.3 x, of every other group of either by under 1.3 x.
        xyz, dens, sc, q = _cloud(20, 508, spread=0.01)
        sc = (5e-4 * np.exp(np.random.RandomState(99).uniform(-np.log(1.25), np.log(1.25), sc.shape))).astype(np.float32)
        g = np.random.RandomState(38)
        aim = xyz[np.arange(200) % 20] + g.randn(200, 3) * 1.5 * 5e-4
        u = g.randn(200, 3)
        u /= np.linalg.norm(u, axis=1, keepdims=True)
        o = (aim - 6.0 * u).astype(np.float32)
        d = ((aim - o) * np.exp(g.uniform(np.log(0.01), np.log(10.0), (200, 1)))).astype(np.float32)
        cloud = (xyz, dens, sc, q)
    elif name == "raw_quat":   # quaternions used as they come: norms 0.3 .. 3
        xyz, dens, sc, q = _cloud(60, 509, lo=0.03, hi=0.3)
        q = (q * np.exp(np.random.RandomState(39).uniform(np.log(0.3), np.log(3.0), (60, 1)))).astype(np.float32)
        cloud, (o, d) = (xyz, dens, sc, q), _lines(200, 40)
    elif name == "singular":   # Gaussian 3: |q|^2 = 1/2 and r = 5e-4, s_min(R)^2 = 2 r^2 < 1e-6: an infinite radius
        # (R is diag(1, 0, 0) up to 7e-4: a slab across x.  Where it alone is seen, d / d start_x is 600 times smaller than along
        # y and z and is normalised by itself, so this scene's e32 of the start gradient is of order 1; the other six are not.)
        xyz, dens, sc, q = (a.copy() for a in _cloud(40, 510, lo=0.03, hi=0.3))
        q[3] = (5e-4, np.sqrt(0.5), 0.0, 0.0)
        cloud, (o, d) = (xyz, dens, sc, q), _lines(200, 41)
    elif name in ("mod_half", "mod_two"):
        cloud, (o, d), mod = _cloud(60, 511, lo=0.03, hi=0.3), _lines(200, 42), {"mod_half": 0.5, "mod_two": 2.0}[name]
    elif name == "bad":
        xyz, dens, sc, q = (a.copy() for a in _cloud(12, 512, lo=0.05, hi=0.3))
        xyz[1, 2], sc[2, 0], sc[3, 1] = np.nan, np.inf, 0.0
        o, d = _lines(64, 43, lo=0.1, hi=10.0)
        o[5, 1], o[9, 0], d[20, 2], d[30, 0], d[41] = np.nan, np.inf, np.nan, -np.inf, 0.0
        cloud, zg, zr = (xyz, dens, sc, q), [1, 2, 3], [5, 9, 20, 30, 41]
    else:
        raise KeyError(name)
    N = o.reshape(-1, 3).shape[0]
    G = (np.random.RandomState(5).rand(N) * 2 - 1).astype(np.float32)
    return {"origins": np.ascontiguousarray(o, np.float32), "directions": np.ascontiguousarray(d, np.float32), "half_line": bool(half),
            "cloud": cloud, "mod": mod, "G": G, "zero_gaussians": zg, "zero_rays": zr}


SCENES = ("flat_cone", "flat_parallel", "scattered") + tuple("tail_%d" % n for n in TAILS) + (
    "many", "none", "curved", "miss", "inside", "offset", "tiny", "offset_tiny", "raw_quat", "singular", "mod_half", "mod_two", "bad")

_CACHE = {}


def reference_of(sc):
    """Float64 results of a scene dictionary: dict(scene, lo, hi: bundle64 with qmax = 32 and None, with G)."""
    args = (sc["origins"], sc["directions"], sc["half_line"]) + tuple(sc["cloud"])
    return {"scene": sc, "lo": bundle64(*args, mod=sc["mod"], qmax=32.0, G=sc["G"]), "hi": bundle64(*args, mod=sc["mod"], G=sc["G"])}


def reference(name):
    """reference_of(scene(name)), computed once per process."""
    if name not in _CACHE:
        _CACHE[name] = reference_of(scene(name))
    return _CACHE[name]


def error_against(ref, got_val, got_grads=None):
    """Worst normalised error of values (and gradients) against a float64 result `ref` of bundle64(..., G=...)."""
    out = {"value": _worst(np.asarray(got_val, np.float64).reshape(-1) - ref["val"], ref["abs"])}
    if got_grads is not None:
        for k in GRADS:
            out[k] = _worst(np.asarray(got_grads[k], np.float64).reshape(ref["grads"][k].shape) - ref["grads"][k], ref["gabs"][k])
    return out


def measure_e32(name):
    r = reference(name)
    sc = r["scene"]
    f32 = bundle32(sc["origins"], sc["directions"], sc["half_line"], *sc["cloud"], mod=sc["mod"], G=sc["G"])
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
