"""What do the Jacobian products of the exact projector cost next to the operators they mirror?  (DESIGN.md section 4,
"Jacobian products and Gauss-Newton".)

    python scripts/gauss_newton_bench.py [--P 50000] [--size 512] [--reps 20] [--out gauss_newton_bench.json]

On a scene.make_cloud cloud, cone beam, one view of a size^2 detector, in one process:

* ``project_gaussians_jvp`` (a tangent of the cloud), next to ``projection_variance`` (the same walk, the same staged record,
  one multiply more per term) and next to the forward;
* ``geometry.ray_jacobian``, next to the ray backward of ``project_gaussians_rays`` (the same walk, plus the reduction);
* ``gauss_newton.normal_matvec``, next to one forward plus one parameter backward;
* one iteration of ``geometry.refine_geometry_lm`` against one of ``geometry.refine_geometry``, both refining offDetector
  on three views of the detector (each includes its host work; the LM iteration reads one comparison back).

Times: the protocol of scripts/uncertainty_bench.py -- one pair of HIP events around every call after three warm-up calls, the
median over `reps` calls with the smallest and the largest.  One process, one run.  Not a test and not a gate.
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from r2_gaussian_amd import gauss_newton as GN                                               # noqa: E402
from r2_gaussian_amd import geometry as GE                                                   # noqa: E402
from r2_gaussian_amd import scene as S                                                       # noqa: E402
from r2_gaussian_amd import uncertainty as U                                                 # noqa: E402
from r2_gaussian_amd.gaussian_projector import (project_gaussians, project_gaussians_jvp, project_gaussians_rays,   # noqa: E402
                                                world_ray_params)
from scripts.field_error import timed                                                        # noqa: E402


def ratio(a, b):
    return a["median_ms"] / b["median_ms"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--P", type=int, default=50000)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default="", help="also write the results to this JSON file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gauss_newton_bench.py measures on the GPU: none visible")
    dev = torch.device("cuda:0")
    cloud = S.make_cloud(a.P, seed=7)
    leaves = [t.to(dev) for t in (cloud.xyz, cloud.density, cloud.scales, cloud.rotations)]
    res = {"P": a.P, "size": a.size}

    def emit(key, value):
        res[key] = value
        print(key, json.dumps(value))
        sys.stdout.flush()

    one = S.make_views(1, (a.size, a.size))
    rays = torch.from_numpy(world_ray_params(one)).to(dev)
    gen = torch.Generator(device="cpu").manual_seed(1)
    tan = tuple((0.01 * torch.randn(t.shape, generator=gen)).to(dev) for t in leaves)
    var = tuple(t * t for t in tan)
    G = torch.rand((1, a.size, a.size), device=dev)
    with torch.no_grad():
        out = {"jvp": timed(lambda: project_gaussians_jvp(one, *leaves, tangents=tan), a.reps, dev),
               "projection_variance": timed(lambda: U.projection_variance(one, *leaves, var), a.reps, dev),
               "project_forward": timed(lambda: project_gaussians(one, *leaves), a.reps, dev)}
    out["jvp_over_variance"] = ratio(out["jvp"], out["projection_variance"])
    out["jvp_over_forward"] = ratio(out["jvp"], out["project_forward"])
    emit("jvp_1_view", out)

    rg = rays.clone().requires_grad_(True)
    img = project_gaussians_rays(rg, True, a.size, a.size, *leaves)
    out = {"ray_jacobian": timed(lambda: GE.ray_jacobian(rays, True, a.size, a.size, *leaves), a.reps, dev),
           "rays_backward": timed(lambda: torch.autograd.grad(img, rg, G, retain_graph=True), a.reps, dev)}
    out["jacobian_over_rays_backward"] = ratio(out["ray_jacobian"], out["rays_backward"])
    emit("ray_jacobian_1_view", out)
    del img

    lg = [t.clone().requires_grad_(True) for t in leaves]

    def forward_backward():
        torch.autograd.grad(project_gaussians_rays(rays, True, a.size, a.size, *lg), lg, G)

    out = {"normal_matvec": timed(lambda: GN.normal_matvec(rays, True, a.size, a.size, leaves, tan), a.reps, dev),
           "forward_plus_backward": timed(forward_backward, a.reps, dev)}
    out["matvec_over_forward_backward"] = ratio(out["normal_matvec"], out["forward_plus_backward"])
    emit("normal_matvec_1_view", out)

    # one iteration of each geometry fit: three views, the detector of the measured projections shifted by 1.5 pixels
    n = (a.size, a.size)
    args = GE.scanner_args(S.CONE_BEAM, n)
    angles = torch.tensor([0.3, 2.4, 4.5], dtype=torch.float64, device=dev)
    true = torch.tensor([-0.9 * args["dDetector"][0], 1.2 * args["dDetector"][1]], dtype=torch.float64, device=dev)
    fn = lambda p: GE.scan_rays(angles, **dict(args, offDetector=p["offDetector"]))
    with torch.no_grad():
        projs = project_gaussians_rays(fn({"offDetector": true}), True, a.size, a.size, *leaves)
    start = {"offDetector": torch.zeros(2, dtype=torch.float64, device=dev)}
    out = {"lm_iteration": timed(lambda: GE.refine_geometry_lm(projs, leaves, fn, start, 1), a.reps, dev),
           "adam_iteration": timed(lambda: GE.refine_geometry(projs, leaves, fn, start, 1, 0.01), a.reps, dev)}
    out["lm_over_adam"] = ratio(out["lm_iteration"], out["adam_iteration"])
    emit("geometry_iteration_3_views", out)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
