"""What does a projection plan cost, and what does it save?  ("Projection plans".)

    python scripts/plan_bench.py [--P 50000] [--size 512] [--views 1 8] [--reps 20] [--out plan_bench.json]

On a scene.make_cloud cloud, cone beam, a size^2 detector, for every number of views given, in one process:

* the plan build, and its count and fill timed separately (the build includes the host read between them);
* the instances per view and the longest list;
* each of the five planned operators next to its unplanned twin -- the forward, the ray backward, the projection variance,
  the JVP, the ray Jacobian -- the two alternating call by call, and torch.equal of their outputs at this size;
* ``gauss_newton.normal_matvec`` planned (its build included) and not;
* one ``gauss_newton.gauss_newton_step`` with cg_iters = 3, planned (its build included) and not;
* the number of forwards after which build + planned forwards beat unplanned forwards.

Times: the protocol of scripts/gauss_newton_bench.py -- one pair of HIP events around every call after three warm-up calls, the
median over `reps` calls with the smallest and the largest.  One process, one run.  Not a test and not a gate.
"""
import argparse
import json
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from r2_gaussian_amd import gauss_newton as GN                                               # noqa: E402
from r2_gaussian_amd import gaussian_projector as GP                                         # noqa: E402
from r2_gaussian_amd import geometry as GE                                                   # noqa: E402
from r2_gaussian_amd import scene as S                                                       # noqa: E402
from r2_gaussian_amd import uncertainty as U                                                 # noqa: E402
from scripts.field_error import timed                                                        # noqa: E402


def timed_pair(planned, unplanned, reps, dev, warm=3):
    """The two callables alternating, every call between its own pair of events -> {"planned": ..., "unplanned": ...,
    "ratio": median planned / median unplanned, "separate": the two ranges do not overlap}."""
    for _ in range(warm):
        planned()
        unplanned()
    torch.cuda.synchronize(dev)
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(4)] for _ in range(reps)]
    for a, b, c, d in ev:
        a.record()
        planned()
        b.record()
        c.record()
        unplanned()
        d.record()
    torch.cuda.synchronize(dev)
    out = {}
    for key, i in (("planned", 0), ("unplanned", 2)):
        t = sorted(e[i].elapsed_time(e[i + 1]) for e in ev)
        out[key] = {"median_ms": t[len(t) // 2], "min_ms": t[0], "max_ms": t[-1], "reps": reps}
    out["ratio"] = out["planned"]["median_ms"] / out["unplanned"]["median_ms"]
    out["separate"] = out["planned"]["max_ms"] < out["unplanned"]["min_ms"] or out["unplanned"]["max_ms"] < out["planned"]["min_ms"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--P", type=int, default=50000)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--views", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default="", help="also write the results to this JSON file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("plan_bench.py measures on the GPU: none visible")
    dev = torch.device("cuda:0")
    cloud = S.make_cloud(a.P, seed=7)
    leaves = [t.to(dev) for t in (cloud.xyz, cloud.density, cloud.scales, cloud.rotations)]
    gen = torch.Generator(device="cpu").manual_seed(1)
    tan = tuple((0.01 * torch.randn(t.shape, generator=gen)).to(dev) for t in leaves)
    var = tuple(t * t for t in tan)
    H = W = a.size
    res = {"P": a.P, "size": a.size}

    def emit(key, value):
        res[key] = value
        print(key, json.dumps(value))
        sys.stdout.flush()

    for V in a.views:
        rays = torch.from_numpy(GP.world_ray_params(S.make_views(V, (H, W)))).to(dev)
        args = (rays, True, H, W, *leaves)
        x, d, s, r = (GP.f32c(t) for t in leaves)
        with torch.no_grad():
            plan = GP.plan_projection_rays(*args)
            offsets, ws = GP._plan_count(rays, 1, H, W, x, d, s, r, 1.0)
            build = {"build": timed(lambda: GP.plan_projection_rays(*args), a.reps, dev),
                     "count": timed(lambda: GP._plan_count(rays, 1, H, W, x, d, s, r, 1.0), a.reps, dev),
                     "fill": timed(lambda: GP._plan_fill(rays, 1, H, W, x, d, s, r, 1.0, offsets, ws, plan.instances), a.reps, dev)}
        sizes = plan.offsets[1:] - plan.offsets[:-1]
        build.update(instances=plan.instances, instances_per_view=plan.instances / V, longest_list=int(sizes.max()),
                     mean_list=float(sizes.double().mean()), tiles_per_view=int(sizes.numel() // V))
        emit("build_%d_views" % V, build)

        G = torch.rand((V, H, W), device=dev)
        ops = {}
        with torch.no_grad():
            pairs = {"forward": (lambda: GP.project_gaussians_rays(*args, plan=plan), lambda: GP.project_gaussians_rays(*args)),
                     "variance": (lambda: U.projection_variance_rays(*args, var, plan=plan),
                                  lambda: U.projection_variance_rays(*args, var)),
                     "jvp": (lambda: GP.project_gaussians_rays_jvp(*args, tangents=tan, plan=plan),
                             lambda: GP.project_gaussians_rays_jvp(*args, tangents=tan)),
                     "ray_jacobian": (lambda: GE.ray_jacobian(*args, plan=plan), lambda: GE.ray_jacobian(*args))}
            for key, (p, u) in pairs.items():
                assert torch.equal(p(), u()), key
                ops[key] = timed_pair(p, u, a.reps, dev)
        rg = rays.clone().requires_grad_(True)
        plan_g = GP.plan_projection_rays(rg, True, H, W, *leaves)
        img_p = GP.project_gaussians_rays(rg, True, H, W, *leaves, plan=plan_g)
        img_u = GP.project_gaussians_rays(rg, True, H, W, *leaves)
        bp = lambda: torch.autograd.grad(img_p, rg, G, retain_graph=True)[0]
        bu = lambda: torch.autograd.grad(img_u, rg, G, retain_graph=True)[0]
        assert torch.equal(bp(), bu())
        ops["rays_backward"] = timed_pair(bp, bu, a.reps, dev)
        del img_p, img_u
        emit("operators_%d_views" % V, ops)

        with torch.no_grad():
            mv = lambda planned: GN.normal_matvec(rays, True, H, W, leaves, tan, planned=planned)
            assert all(torch.equal(p, u) for p, u in zip(mv(True), mv(False)))
            emit("normal_matvec_%d_views" % V, timed_pair(lambda: mv(True), lambda: mv(False), a.reps, dev))
            projs = GP.project_gaussians_rays(*args) * 1.05
            step = lambda planned: GN.gauss_newton_step(rays, True, H, W, leaves, projs, 3, 1e-3, planned=planned)
            (cp, lp), (cu, lu) = step(True), step(False)
            assert torch.equal(lp, lu) and all(torch.equal(p, u) for p, u in zip(cp, cu))
            emit("gauss_newton_step_cg3_%d_views" % V, timed_pair(lambda: step(True), lambda: step(False), a.reps, dev))

        f = ops["forward"]
        saved = f["unplanned"]["median_ms"] - f["planned"]["median_ms"]
        emit("break_even_%d_views" % V, {"build_ms": build["build"]["median_ms"], "saved_per_forward_ms": saved,
                                         "forwards": math.ceil(build["build"]["median_ms"] / saved) if saved > 0 else None})
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
