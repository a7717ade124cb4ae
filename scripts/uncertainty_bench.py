"""What do the Fisher diagonal and the predictive variances cost next to the operators they square?  (DESIGN.md section 4,
"Fisher information and predictive variance".)

    python scripts/uncertainty_bench.py [--P 50000] [--size 512] [--views 50] [--reps 20] [--out uncertainty_bench.json]

On a scene.make_cloud cloud, cone beam, size^2 detector:

* ``fisher_diagonal`` on one view and on `views` views, next to the parameter backward of ``project_gaussians`` on the same
  views (the yardstick: the same walk over the same pairs, plus eleven multiplies per pair);
* ``field_variance`` on a size^2 oblique plane and a 32^3 patch, next to ``query_points`` forward;
* ``projection_variance`` on one view, next to ``project_gaussians`` forward.

Times: the protocol of scripts/field_error.py -- one pair of HIP events around every call after three warm-up calls, the median
over `reps` calls with the smallest and the largest.  One process, one run.  Not a test and not a gate.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from r2_gaussian_amd import scene as S                                                       # noqa: E402
from r2_gaussian_amd import uncertainty as U                                                 # noqa: E402
from r2_gaussian_amd.field import plane_points, query_points, voxel_centres                  # noqa: E402
from r2_gaussian_amd.gaussian_projector import project_gaussians                             # noqa: E402
from scripts.field_error import timed                                                        # noqa: E402


def ratio(a, b):
    return a["median_ms"] / b["median_ms"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--P", type=int, default=50000)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--views", type=int, default=50)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default="", help="also write the results to this JSON file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("uncertainty_bench.py measures on the GPU: none visible")
    dev = torch.device("cuda:0")
    cloud = S.make_cloud(a.P, seed=7)
    leaves = [t.to(dev) for t in (cloud.xyz, cloud.density, cloud.scales, cloud.rotations)]
    res = {"P": a.P, "size": a.size}

    def emit(key, value):
        res[key] = value
        print(key, json.dumps(value))
        sys.stdout.flush()

    for V in (1, a.views):
        views = S.make_views(V, (a.size, a.size))
        G = torch.rand((V, a.size, a.size), device=dev)
        lg = [t.clone().requires_grad_(True) for t in leaves]
        img = project_gaussians(views, *lg)
        out = {"fisher": timed(lambda: U.fisher_diagonal(views, *leaves), a.reps, dev),
               "project_backward": timed(lambda: torch.autograd.grad(img, lg, G, retain_graph=True), a.reps, dev)}
        out["fisher_over_backward"] = ratio(out["fisher"], out["project_backward"])
        emit("views_%d" % V, out)
        del img

    var = U.parameter_variance(U.fisher_diagonal(S.make_views(a.views, (a.size, a.size)), *leaves), 1e-3)
    d = 1.8 / a.size   # the oblique plane of scripts/field_error.py
    u = np.array([0.8, 0.5, 0.33]) / np.linalg.norm([0.8, 0.5, 0.33]) * d
    v = np.cross([0.2, -0.7, 0.68], u)
    v = v / np.linalg.norm(v) * d
    sets = {"plane_%d" % a.size: plane_points(-(u + v) * a.size / 2, u, v, a.size, a.size, dev),
            "patch_32": voxel_centres((0.1, -0.1, 0.0), (32, 32, 32), (0.25, 0.25, 0.25), dev)}
    with torch.no_grad():
        for name, pts in sets.items():
            out = {"field_variance": timed(lambda: U.field_variance(pts, *leaves, var), a.reps, dev),
                   "query_points": timed(lambda: query_points(pts, *leaves), a.reps, dev)}
            out["variance_over_query"] = ratio(out["field_variance"], out["query_points"])
            emit(name, out)
        one = S.make_views(1, (a.size, a.size))
        out = {"projection_variance": timed(lambda: U.projection_variance(one, *leaves, var), a.reps, dev),
               "project_forward": timed(lambda: project_gaussians(one, *leaves), a.reps, dev)}
        out["variance_over_forward"] = ratio(out["projection_variance"], out["project_forward"])
        emit("projection_1_view", out)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
