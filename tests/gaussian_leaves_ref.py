"""The scenes of the leaf-culled exact line integrals (include/r2hip.h: r2_integrate_gaussians_leaves and its backward;
csrc/gaussian_leaves.hpp), the measured float32 error their GPU tolerance is taken from, and the float32 restatement of what
the leaf culling adds: the prepare kernel (the radius of every Gaussian, the box of every leaf of 64) and the leaf test (the
slab test of a ray against a leaf's box), in the header's operation order.  Host only; the product never imports this file.

The contract of a pair, the float64 reference, the float32 restatement of the sums and the error measure are
tests/gaussian_bundle_ref.py's, imported, not copied: the rule that decides which pairs are summed is the same, and the
leaves only cull in front of it.

tests/golden/gaussian_leaves/e32.json holds ``measure_e32`` of every scene below (written by
``python -m tests.gaussian_leaves_ref``); the GPU tests allow 4 x that, as the sibling tests do.
"""
import json
import os

import numpy as np

from tests import gaussian_project_ref as R
from tests.gaussian_bundle_ref import (_cloud, _lines, bundle32, bundle64, error_against, reference_of, valid_gaussians,  # noqa: F401
                                       valid_rays)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gaussian_leaves", "e32.json")
LEAF = 64
F = np.float32
GB_EPS = F(2.0 ** -20)
GQ_CUT = F(32.001)
GP_SPHERE = F(F(5.656854249492381) * F(1.01))

# The stochastic refinement (geometry.refine_geometry(rays_per_step=...)) on gaussian_project_rays_ref.refine_setup(): a
# quarter of its 3 x 17 x 23 pixels per step, the K steps and learning rate of that module.
REFINE_RAYS, REFINE_SEED = 293, 0


# ------------------------------------------------------------------------------------------------------ the scenes
LEAF_TAILS = (1, 63, 64, 65, 129)


def ordered(cloud, mod=1.0):
    """The cloud permuted by the product's cloud_order (on the host)."""
    import torch
    from r2_gaussian_amd.gaussian_projector import cloud_order
    perm = cloud_order(torch.from_numpy(cloud[0]), torch.from_numpy(cloud[2]), mod).numpy()
    return tuple(np.ascontiguousarray(a[perm]) for a in cloud)


def _spread():
    return _cloud(1500, 601, lo=0.01, hi=0.03, spread=1.0)


def _mixed():
    xyz, dens, sc, q = (a.copy() for a in _spread())
    big = np.random.RandomState(602).permutation(1500)[:30]
    sc[big] *= F(20.0)
    return xyz, dens, sc, q


def scene(name):
    """-> the dictionary of gaussian_bundle_ref.scene."""
    half = False
    if name.startswith("leaf_tail_"):   # P = 1, 63, 64, 65, 129: a partial leaf, a full one, a full one and one Gaussian, ...
        P = int(name[10:])
        cloud, (o, d) = _cloud(P, 610 + P, lo=0.03, hi=0.3), _lines(70, 50)
    elif name == "spread":   # 23 full leaves and one of 28, in random index order: every leaf box spans the cloud
        cloud, (o, d) = _spread(), _lines(600, 51, half=1.0)
    elif name == "spread_ordered":   # the same cloud in cloud_order: compact leaves, most (ray, leaf) pairs culled
        cloud, (o, d) = ordered(_spread()), _lines(600, 51, half=1.0)
    elif name == "mixed":   # 30 of the Gaussians 20 x larger, ordered
        cloud, (o, d) = ordered(_mixed()), _lines(600, 51, half=1.0)
    elif name == "one_pair":   # a 28 x 25 lattice of pitch 0.5 in z = 0, sigma = 0.01: no line parallel to z meets two spheres
        # Along z every derivative with respect to a mean or a ray is analytically zero: the float64 reference holds the
        # rounding noise of a cancelling sum there, the measured e32 of those three groups is noise over noise (1e11) and their
        # bracket says nothing; this scene's check is the bit-equality with method="blocks".  Where float64 happens to cancel
        # to an exact 0 the bracket would hold float32's noise against the underflow floor, so the seed is one for which no
        # component has a float64 denominator under FLOOR and a non-zero float32 restatement (the CPU tests assert it).
        g = np.random.RandomState(604)
        ix, iy = np.meshgrid(np.arange(28), np.arange(25), indexing="ij")
        xyz = np.stack([(ix.reshape(-1) - 13.5) * 0.5, (iy.reshape(-1) - 12.0) * 0.5, np.zeros(700)], 1)
        q = g.randn(700, 4)
        q /= np.linalg.norm(q, axis=1, keepdims=True)
        cloud = tuple(a.astype(F) for a in (xyz, 0.1 + 0.9 * g.rand(700, 1), np.full((700, 3), 0.01), q))
        through = xyz[g.randint(700, size=300)] + np.concatenate([g.randn(300, 2) * 0.012, np.zeros((300, 1))], 1)
        d = np.zeros((300, 3))
        d[:, 2] = np.where(g.rand(300) < 0.5, -1.0, 1.0) * np.exp(g.uniform(np.log(0.01), np.log(100.0), 300))
        o = through - d / np.abs(d[:, 2:3]) * (1.0 + 3.0 * g.rand(300, 1))
        o, d = o.astype(F), d.astype(F)
    else:
        raise KeyError(name)
    N = o.shape[0]
    G = (np.random.RandomState(5).rand(N) * 2 - 1).astype(F)
    return {"origins": np.ascontiguousarray(o, F), "directions": np.ascontiguousarray(d, F), "half_line": bool(half),
            "cloud": cloud, "mod": 1.0, "G": G, "zero_gaussians": [], "zero_rays": []}


SCENES = tuple("leaf_tail_%d" % p for p in LEAF_TAILS) + ("spread", "spread_ordered", "mixed", "one_pair")

_CACHE = {}


def reference(name):
    """gaussian_bundle_ref.reference_of(scene(name)), computed once per process."""
    if name not in _CACHE:
        _CACHE[name] = reference_of(scene(name))
    return _CACHE[name]


def measure_e32(name):
    """As gaussian_bundle_ref.measure_e32 measures it: the float32 restatement of the sums against float64, every pair."""
    r = reference(name)
    sc = r["scene"]
    f32 = bundle32(sc["origins"], sc["directions"], sc["half_line"], *sc["cloud"], mod=sc["mod"], G=sc["G"])
    return error_against(r["hi"], f32["val"], f32["grads"])


def load_e32():
    with open(GOLDEN) as f:
        return json.load(f)


# ------------------------------------------------------------------------------------------------------ the leaf restatement
def radius32(xyz, density, scaling, rotation, mod=1.0):
    """[P] float32: gauss_radius (csrc/gaussian_rays.hpp), one rounded float32 operation per step in its order; -1 for a
    Gaussian that contributes nothing, inf for a nearly singular rotation."""
    P = np.asarray(xyz).shape[0]
    m, s, q = np.asarray(xyz, F).reshape(P, 3), np.asarray(scaling, F).reshape(P, 3), np.asarray(rotation, F).reshape(P, 4)
    rho, mod = np.asarray(density, F).reshape(P), F(mod)
    with np.errstate(all="ignore"):
        tot = m[:, 0] + m[:, 1] + m[:, 2] + rho + s[:, 0] + s[:, 1] + s[:, 2] + mod + q[:, 0] + q[:, 1] + q[:, 2] + q[:, 3]
        s0, s1, s2 = s[:, 0] * mod, s[:, 1] * mod, s[:, 2] * mod
        dead = ~(np.abs(tot) < np.inf) | ~(s0 > 0) | ~(s1 > 0) | ~(s2 > 0)
        n2 = q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1] + q[:, 2] * q[:, 2] + q[:, 3] * q[:, 3]
        om = F(1.0) - n2
        e2 = om * om + F(2.0) * om * (F(2.0) * q[:, 0] * q[:, 0] - n2) + n2 * n2
        smin2 = np.minimum(F(1.0), e2)
        r = GP_SPHERE * np.maximum(s0, np.maximum(s1, s2)) / np.sqrt(smin2)
        r = np.where(smin2 > F(1e-6), r, F(np.inf))
    return np.where(dead, F(-1.0), r).astype(F)


def leaf_boxes32(xyz, radius):
    """(lo, hi) [L,3] float32: the prepare kernel's leaf boxes, the bounding box of mu -+ radius over the members of each leaf of
    64 consecutive Gaussians with radius >= 0 (lo = +inf, hi = -inf for a leaf without any)."""
    m = np.asarray(xyz, F)
    P = m.shape[0]
    L = (P + LEAF - 1) // LEAF
    lo, hi = np.full((L * LEAF, 3), np.inf, F), np.full((L * LEAF, 3), -np.inf, F)
    live = radius >= 0
    with np.errstate(all="ignore"):
        lo[:P][live] = m[live] - radius[live, None]
        hi[:P][live] = m[live] + radius[live, None]
    return lo.reshape(L, LEAF, 3).min(1), hi.reshape(L, LEAF, 3).max(1)


def rays_meet_leaves32(origins, directions, half_line, lo, hi):
    """[N,L] bool: the leaf test, bundle_ray_box's return value (csrc/gaussian_bundle.hpp (1)) with a leaf's box in the place
    of the cloud box, one rounded float32 operation per step in its order."""
    o, d = np.asarray(origins, F).reshape(-1, 3), np.asarray(directions, F).reshape(-1, 3)
    valid = valid_rays(o, d)
    with np.errstate(all="ignore"):
        length = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])
        l2 = length * length
        tame = valid & (l2 >= F(1e-30)) & (l2 <= F(1e30))
        h = np.where(tame[:, None], d / np.where(tame, length, F(1.0))[:, None], F(0.0)).astype(F)
        N, L = o.shape[0], lo.shape[0]
        t0 = np.full((N, L), F(0.0) if half_line else F(-np.inf), F)
        t1 = np.full((N, L), np.inf, F)
        miss = np.zeros((N, L), bool)
        for k in range(3):
            blo = (lo[:, k] - GB_EPS * np.abs(lo[:, k]))[None, :]
            bhi = (hi[:, k] + GB_EPS * np.abs(hi[:, k]))[None, :]
            s, hk = o[:, k:k + 1], h[:, k:k + 1]
            flat = hk == 0
            miss |= flat & ((s < blo) | (s > bhi))
            hs = np.where(flat, F(1.0), hk)
            ta, tb = (blo - s) / hs, (bhi - s) / hs
            a, c = np.minimum(ta, tb), np.maximum(ta, tb)
            t0 = np.where(flat, t0, np.maximum(t0, a - GB_EPS * np.abs(a)))
            t1 = np.where(flat, t1, np.minimum(t1, c + GB_EPS * np.abs(c)))
        meets = np.where(tame[:, None], ~miss & (t0 <= t1), True)
    return meets & valid[:, None] & (lo[:, 0] <= hi[:, 0])[None, :]


def summed32(origins, directions, half_line, xyz, density, scaling, rotation, mod=1.0):
    """[N,P] bool: the pairs the rule sums, decided in float32 as the kernels decide it: a valid ray, a Gaussian with
    gauss_radius >= 0, the pair accepted (gaussian_project_ref.contract's keep) and its q, formed from wp, <= 32.001."""
    o, d = np.asarray(origins, F).reshape(-1, 3), np.asarray(directions, F).reshape(-1, 3)
    P = np.asarray(xyz).shape[0]
    cols = lambda a, c: R._cols(np.asarray(a, F).reshape(P, c), F)
    ok = valid_rays(o, d)[:, None] & valid_gaussians(xyz, density, scaling, rotation, mod)[None, :]
    with np.errstate(all="ignore"):
        c = R.contract(np, [o[:, j:j + 1] for j in range(3)], [d[:, j:j + 1] for j in range(3)], half_line, cols(xyz, 3),
                       cols(density, 1)[0], cols(scaling, 3), F(mod), cols(rotation, 4), GQ_CUT)
    return c["keep"] & ok


def culled_summed_pairs(sc):
    """-> (number of pairs the rule sums, number of those whose leaf the leaf test culls or whose radius is negative, share of
    (ray, leaf) pairs the test keeps) for a scene dictionary."""
    cloud, mod = sc["cloud"], sc["mod"]
    r = radius32(*cloud, mod=mod)
    lo, hi = leaf_boxes32(cloud[0], r)
    meets = rays_meet_leaves32(sc["origins"], sc["directions"], sc["half_line"], lo, hi)
    summed = summed32(sc["origins"], sc["directions"], sc["half_line"], *cloud, mod=mod)
    P = cloud[0].shape[0]
    per_gaussian = np.repeat(meets, LEAF, axis=1)[:, :P] & (r >= 0)[None, :]
    return int(summed.sum()), int((summed & ~per_gaussian).sum()), float(meets.mean()) if meets.size else 0.0


# ------------------------------------------------------------------------------------------------------ the stochastic refinement
def refine_host_subset(setup, K, lr, rays_per_step=REFINE_RAYS, seed=REFINE_SEED):
    """refine_geometry(rays_per_step=...)'s loop on the host in float64: the same draws (torch.randperm of a CPU generator
    seeded once), scan_rays and pixel_rays of the product in float64, the pair under autograd (gaussian_bundle_ref.torch_bundle),
    torch.optim.Adam.  -> (offDetector [2] float64, loss history [K])."""
    import torch
    from r2_gaussian_amd import geometry
    from tests import gaussian_project_rays_ref as Q
    from tests.gaussian_bundle_ref import torch_bundle
    fn = Q.refine_rays_fn(setup)
    H, W = setup["H"], setup["W"]
    target = torch.from_numpy(setup["projs"].astype(np.float64)).reshape(-1)
    total = target.numel()
    cloud = [torch.from_numpy(np.asarray(a, np.float64)) for a in setup["cloud"]]
    p = torch.zeros(2, dtype=torch.float64, requires_grad=True)
    opt = torch.optim.Adam([p], lr=lr, betas=geometry.ADAM_BETAS, eps=geometry.ADAM_EPS)
    gen = torch.Generator(device="cpu").manual_seed(int(seed))
    hist = []
    for _ in range(K):
        opt.zero_grad(set_to_none=True)
        pick = torch.randperm(total, generator=gen)[:rays_per_step]
        view = pick // (H * W)
        rest = pick - view * (H * W)
        row = rest // W
        col = rest - row * W
        o, d = geometry.pixel_rays(fn({"offDetector": p})[view], True, H, W, row[:, None], col[:, None])
        diff = torch_bundle(o.reshape(-1, 3), d.reshape(-1, 3), True, *cloud) - target[pick]
        value = (diff * diff).mean()
        value.backward()
        opt.step()
        hist.append(float(value.detach()))
    return p.detach().numpy().copy(), hist


if __name__ == "__main__":
    os.makedirs(os.path.dirname(GOLDEN), exist_ok=True)
    res = {n: measure_e32(n) for n in SCENES}
    with open(GOLDEN, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    for n, v in res.items():
        print(n, " ".join("%s %.3e" % kv for kv in v.items()))
