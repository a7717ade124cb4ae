"""Restatement of the ray gradient of the exact Gaussian projector (include/r2hip.h: r2_project_gaussians_rays_backward;
csrc/gaussian_ray_grad.hpp), the scenes its tests share, the measured float32 error the GPU tolerance is taken from, and the
host loops the refinement test is held against.  Host only; the product never imports this file.

The pair, the scenes and the float32 floor are tests/gaussian_project_ref.py's (``contract`` decides which pairs are kept);
what is added here is the arithmetic of gaussian_ray_grad.hpp, written component by component in its operation order with
nothing but + - * / sqrt exp, in numpy at a given dtype: float64 is the reference (``qmax`` cuts the sums at q <= qmax, None
sums every pair), float32 rounds once per operation as the kernels do (they are built without FMA contraction).

``ray_grad`` -> the twelve numbers per view and, per component, the sum over pixels and pairs of |contribution|: for pu / pv
with the pixel's c / r weight, for the cone source a = |g_s| + |g_d|.  ``measure_e32`` is the worst |f32 - f64| / that sum over
a scene's components; tests/golden/gaussian_project_rays/e32.json holds it (written by
``python -m tests.gaussian_project_rays_ref``, which also writes refine.json); the GPU tests allow 4 x that.
"""
import json
import os

import numpy as np

from tests import gaussian_project_ref as R

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gaussian_project_rays")
GOLDEN = os.path.join(GOLDEN_DIR, "e32.json")
REFINE_GOLDEN = os.path.join(GOLDEN_DIR, "refine.json")
FLOOR = R.FLOOR

WIDE = ("cone_wide", "parallel_wide")   # 17 x 17 = 289 tiles: more tile partials than the reduce kernel has threads
SCENES = tuple(R.SCENES) + WIDE


def scene(name):
    """gaussian_project_ref.scene, plus `wide` in both beams: detector 260 x 264, P = 7, V = 2."""
    if name not in WIDE:
        return R.scene(name)
    from r2_gaussian_amd import projector
    beam = name.split("_", 1)[0]
    views = R._views(beam, 2, (260, 264))
    rays = projector.ray_params(views, (1.0, 1.0, 1.0), (0.0, 0.0, 0.0), (1, 1, 1))
    G = (np.random.RandomState(6).rand(2, 260, 264) * 2 - 1).astype(np.float32)
    return {"views": views, "rays": rays, "cone": beam == "cone", "H": 260, "W": 264, "cloud": R._cloud(7, 207), "mod": 1.0,
            "G": G, "zero": []}


# ------------------------------------------------------------------------------------------------------ the contract
def pixel_rays(rays, cone, H, W, dtype):
    """pixel_ray (csrc/ray_sampling.hpp) for every pixel of every view in `dtype` arithmetic; `rays` [V,12] is cast to `dtype`
    as it is (float32 parameters are exact in both).  -> s, d: three [V,H,W] arrays each, and fc, fr [1,H,W]-broadcastable."""
    Rr = np.asarray(rays).astype(dtype)[:, None, None, :]
    fc = np.arange(W).astype(dtype)[None, None, :]
    fr = np.arange(H).astype(dtype)[None, :, None]
    p = [Rr[..., 3 + j] + fc * Rr[..., 6 + j] + fr * Rr[..., 9 + j] for j in range(3)]
    a = [np.broadcast_to(Rr[..., j], p[0].shape) for j in range(3)]
    if cone:
        return a, [p[j] - a[j] for j in range(3)], fc, fr
    return p, a, fc, fr


def pair_ray_grad(s, d, cone, mu, rho, scale, mod, quat, G, qmax=None):
    """gauss_pair_ray_grad for all pairs of N rays and P Gaussians (shapes as gaussian_project_ref.contract) -> term [N,P],
    g_s, g_d: three [N,P] arrays each, zero where the pair is not summed."""
    o = R.contract(np, s, d, cone, mu, rho, scale, mod, quat, qmax)
    keep = o["keep"]
    Rm = R._rot(quat)
    isg = [1.0 / (scale[i] * mod) for i in range(3)]
    M = [[Rm[j][i] * isg[i] for j in range(3)] for i in range(3)]
    e = [s[j] - mu[j] for j in range(3)]
    u = [M[i][0] * d[0] + M[i][1] * d[1] + M[i][2] * d[2] for i in range(3)]
    w = [M[i][0] * e[0] + M[i][1] * e[1] + M[i][2] * e[2] for i in range(3)]
    A = u[0] * u[0] + u[1] * u[1] + u[2] * u[2]
    B = u[0] * w[0] + u[1] * w[1] + u[2] * w[2]
    k = B / A
    wp = [w[i] - k * u[i] for i in range(3)]
    q = wp[0] * wp[0] + wp[1] * wp[1] + wp[2] * wp[2]
    t0 = np.sqrt(R.TWO_PI / A) * np.exp(-0.5 * q)
    length = np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
    T = rho * t0
    gl = G * length
    gt = (G * T) / length
    gw = [-(T * wp[i]) for i in range(3)]
    gu = [T * (k * wp[i] - u[i] / A) for i in range(3)]
    gs = [gl * (M[0][j] * gw[0] + M[1][j] * gw[1] + M[2][j] * gw[2]) for j in range(3)]
    gd = [gl * (M[0][j] * gu[0] + M[1][j] * gu[1] + M[2][j] * gu[2]) + gt * d[j] for j in range(3)]
    z = np.zeros_like(o["term"])
    return o["term"], [np.where(keep, c, z) for c in gs], [np.where(keep, c, z) for c in gd]


def ray_grad(dtype, rays, cone, H, W, xyz, density, scaling, rotation, mod=1.0, qmax=None, G=None):
    """-> dict(img [V,H,W], grad [V,12], gabs [V,12]) in `dtype`: the forward image, dL/drays for the pixel gradients G
    [V,H,W], and the sum of |pair contributions| per component."""
    V, P = np.asarray(rays).shape[0], np.asarray(xyz).shape[0]
    S, Dr, fc, fr = pixel_rays(rays, cone, H, W, dtype)
    mu, sc, qt = R._cols(xyz, dtype), R._cols(scaling, dtype), R._cols(rotation, dtype)
    rho = R._cols(np.asarray(density).reshape(P, 1), dtype)[0]
    mod = dtype(mod)
    fc = np.broadcast_to(fc, (1, H, W)).reshape(-1, 1)
    fr = np.broadcast_to(fr, (1, H, W)).reshape(-1, 1)
    img = np.zeros((V, H * W), dtype)
    grad, gabs = np.zeros((V, 12), dtype), np.zeros((V, 12), dtype)
    if P == 0:
        return {"img": img.reshape(V, H, W), "grad": grad, "gabs": gabs}
    Gd = np.asarray(G).astype(dtype)
    step = H * W if H * W * P <= (1 << 21) else max(1, (1 << 21) // P)   # pixels per piece (memory)
    with np.errstate(all="ignore"):
        for v in range(V):
            for a in range(0, H * W, step):
                s = [S[j][v].reshape(-1, 1)[a:a + step] for j in range(3)]
                d = [Dr[j][v].reshape(-1, 1)[a:a + step] for j in range(3)]
                term, gs, gd = pair_ray_grad(s, d, cone, mu, rho, sc, mod, qt, Gd[v].reshape(-1, 1)[a:a + step], qmax)
                img[v, a:a + step] = term.sum(1)
                c, r = fc[a:a + step, 0], fr[a:a + step, 0]
                for j in range(3):
                    ps, pd = gs[j].sum(1), gd[j].sum(1)                      # the pixel's sums over its pairs
                    As, Ad = np.abs(gs[j]).sum(1), np.abs(gd[j]).sum(1)
                    gP, ga = (pd, ps - pd) if cone else (ps, pd)
                    aP, aa = (Ad, As + Ad) if cone else (As, Ad)
                    for off, val, ab in ((0, ga, aa), (3, gP, aP), (6, c * gP, c * aP), (9, r * gP, r * aP)):
                        grad[v, off + j] += val.sum()
                        gabs[v, off + j] += ab.sum()
    return {"img": img.reshape(V, H, W), "grad": grad, "gabs": gabs}


def torch_ray_grad(rays, cone, H, W, xyz, density, scaling, rotation, mod, G):
    """dL/drays [V,12] by torch autograd (float64) through gaussian_project_ref.contract, L = sum(G * image)."""
    import torch
    t = torch.from_numpy(np.asarray(rays, np.float64)).requires_grad_(True)
    fc = torch.arange(W, dtype=torch.float64)[None, None, :]
    fr = torch.arange(H, dtype=torch.float64)[None, :, None]
    Rr = t[:, None, None, :]
    p = [Rr[..., 3 + j] + fc * Rr[..., 6 + j] + fr * Rr[..., 9 + j] for j in range(3)]
    a = [Rr[..., j].expand_as(p[0]) for j in range(3)]
    S, Dr = (a, [p[j] - a[j] for j in range(3)]) if cone else (p, a)
    cols = lambda arr: [torch.from_numpy(c) for c in R._cols(arr, np.float64)]
    loss = 0.0
    for v in range(t.shape[0]):
        s = [S[j][v].reshape(-1, 1) for j in range(3)]
        d = [Dr[j][v].reshape(-1, 1) for j in range(3)]
        o = R.contract(torch, s, d, cone, cols(xyz), cols(density.reshape(-1, 1))[0], cols(scaling), mod, cols(rotation))
        loss = loss + (o["term"].sum(1) * torch.from_numpy(np.asarray(G[v], np.float64)).reshape(-1)).sum()
    loss.backward()
    return t.grad.numpy()


_CACHE = {}


def reference(name):
    """Float64 results of a scene, computed once per process: dict(scene, lo, hi: ray_grad with qmax = 32 and None)."""
    if name not in _CACHE:
        sc = scene(name)
        args = (sc["rays"], sc["cone"], sc["H"], sc["W"]) + sc["cloud"]
        _CACHE[name] = {"scene": sc, "lo": ray_grad(np.float64, *args, mod=sc["mod"], qmax=32.0, G=sc["G"]),
                        "hi": ray_grad(np.float64, *args, mod=sc["mod"], qmax=None, G=sc["G"])}
    return _CACHE[name]


def measure_e32(name):
    """Worst |f32 - f64| / sum |contrib| over the scene's V x 12 components (those under FLOOR are left out)."""
    r = reference(name)
    sc = r["scene"]
    f32 = ray_grad(np.float32, sc["rays"], sc["cone"], sc["H"], sc["W"], *sc["cloud"], mod=sc["mod"], G=sc["G"])
    return R._worst(f32["grad"].astype(np.float64) - r["hi"]["grad"], r["hi"]["gabs"])


def load_e32():
    with open(GOLDEN) as f:
        return json.load(f)


# ------------------------------------------------------------------------------------------------------ the refinement
# cone_p7's geometry (17 x 23, V = 3, DSO 5, DSD 7); the measured projections come from a detector shifted by (-0.9, 1.2)
# pixels (rows, columns): 1.5 pixels.  K steps of Adam at learning rate LR from offDetector = 0.
REFINE_K, REFINE_LR = 60, 0.01
REFINE_SHIFT_PIXELS = (-0.9, 1.2)


def refine_setup():
    """-> dict(args: scan_rays keywords of cone_p7, angles, true: the true offDetector, cloud, H, W, projs: the float64
    exact projection of the shifted geometry rounded to float32)."""
    import torch
    from r2_gaussian_amd import geometry, scene as S
    sc = R.scene("cone_p7")
    H, W = sc["H"], sc["W"]
    args = geometry.scanner_args(dict(S.CONE_BEAM, DSO=5.0, DSD=7.0), (H, W))
    angles = [v.angle for v in sc["views"]]
    true = (REFINE_SHIFT_PIXELS[0] * args["dDetector"][0], REFINE_SHIFT_PIXELS[1] * args["dDetector"][1])
    rays = geometry.scan_rays(torch.tensor(angles, dtype=torch.float64), **dict(args, offDetector=true)).numpy()
    projs = ray_grad(np.float64, rays, True, H, W, *sc["cloud"], G=np.zeros((len(angles), H, W)))["img"].astype(np.float32)
    return {"args": args, "angles": angles, "true": true, "cloud": sc["cloud"], "H": H, "W": W, "projs": projs}


def refine_rays_fn(setup, device=None):
    """The rays_fn of the refinement: params {"offDetector": tensor [2]} -> scan_rays of the setup's geometry."""
    import torch
    from r2_gaussian_amd import geometry
    angles = torch.tensor(setup["angles"], dtype=torch.float64, device=device)
    return lambda p: geometry.scan_rays(angles, **dict(setup["args"], offDetector=p["offDetector"]))


def refine_host(setup, dtype, K=REFINE_K, lr=REFINE_LR):
    """refine_geometry's loop on the host: the projection and its ray gradient in numpy at `dtype` (float32: the rays are
    rounded to float32 first, as the kernels receive them), the mean-squared-error loss and its pixel gradient in `dtype`,
    scan_rays and its chain rule in torch float64 as in the product, and Adam (torch.optim.Adam's update, betas 0.9 / 0.999,
    eps 1e-8) written out in float64.  -> (offDetector [2] float64, loss history [K])."""
    import torch
    from r2_gaussian_amd.geometry import ADAM_BETAS, ADAM_EPS
    fn = refine_rays_fn(setup)
    H, W = setup["H"], setup["W"]
    target = setup["projs"].astype(dtype)
    p = np.zeros(2)
    m, v = np.zeros(2), np.zeros(2)
    b1, b2 = ADAM_BETAS
    hist = []
    for t in range(1, K + 1):
        pt = torch.from_numpy(p.copy()).requires_grad_(True)
        rays = fn({"offDetector": pt})
        rn = rays.detach().numpy()
        if dtype == np.float32:
            rn = rn.astype(np.float32)
        diff = ray_grad(dtype, rn, True, H, W, *setup["cloud"], G=np.zeros(target.shape))["img"] - target
        hist.append(float((diff * diff).mean(dtype=dtype)))
        g0 = dtype(1.0) / dtype(diff.size)
        G = g0 * diff + g0 * diff
        gr = ray_grad(dtype, rn, True, H, W, *setup["cloud"], G=G)["grad"].astype(np.float64)
        rays.backward(torch.from_numpy(gr))
        g = pt.grad.numpy()
        m = b1 * m + (1 - b1) * g
        v = b2 * v + (1 - b2) * g * g
        p = p - (lr / (1 - b1 ** t)) * m / (np.sqrt(v) / np.sqrt(1 - b2 ** t) + ADAM_EPS)
    return p, hist


def measure_refine():
    st = refine_setup()
    p64, h64 = refine_host(st, np.float64)
    p32, _ = refine_host(st, np.float32)
    true = np.asarray(st["true"])
    return {"K": REFINE_K, "lr": REFINE_LR, "true_offDetector": list(map(float, true)),
            "final64": list(map(float, p64)), "final32": list(map(float, p32)),
            "f32_minus_f64": float(np.abs(p32 - p64).max()),
            "initial_error64": float(np.abs(true).max()), "final_error64": float(np.abs(p64 - true).max()),
            "initial_loss64": h64[0], "final_loss64": h64[-1]}


def load_refine():
    with open(REFINE_GOLDEN) as f:
        return json.load(f)


if __name__ == "__main__":
    os.makedirs(GOLDEN_DIR, exist_ok=True)
    res = {n: measure_e32(n) for n in SCENES}
    with open(GOLDEN, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    for n, val in res.items():
        print(n, "%.3e" % val)
    ref = measure_refine()
    with open(REFINE_GOLDEN, "w") as f:
        json.dump(ref, f, indent=1, sort_keys=True)
    print(ref)
