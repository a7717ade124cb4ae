"""What does the exact projector's ray gradient cost, and how well does refine_geometry recover a disturbed scan geometry?
("Ray gradients of the exact projector".)

    python scripts/geometry_error.py [--P 50000] [--size 512] [--views 8] [--iters 300] [--out geometry_error.json]

Times: one pair of HIP events around every call after a warm-up; the median over `reps` calls with the smallest and the
largest, for one view of size^2 pixels and a scene.make_cloud cloud of P Gaussians in both beams: the forward alone, and
forward + ray backward (only the rays require grad, so the parameter backward is not launched).

Recovery: the same cloud on `views` views of rec_size^2 pixels, cone beam.  The measured projections come from a detector
shifted in its plane, rolled about its normal, and from jittered angles; refine_geometry starts from the nominal geometry and
refines offDetector (2), roll (1) and d_angle (per view).  Reported: the error of every parameter before and after, in pixels
and radians, and the loss before and after.  A common angle offset is not observable (it turns the object about the axis), so
the jitter has zero mean and the angle error is reported after removing its mean.  Not a test and not a gate.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from r2_gaussian_amd import geometry                                           # noqa: E402
from r2_gaussian_amd import scene as S                                         # noqa: E402
from r2_gaussian_amd.gaussian_projector import project_gaussians_rays          # noqa: E402


def timed(fn, reps, dev, warm=3):
    """-> dict(median_ms, min_ms, max_ms, reps): every call between its own pair of events."""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize(dev)
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize(dev)
    t = sorted(a.elapsed_time(b) for a, b in ev)
    return {"median_ms": t[len(t) // 2], "min_ms": t[0], "max_ms": t[-1], "reps": reps}


def times(leaves, size, dev, reps):
    out = {}
    for scanner in (S.CONE_BEAM, S.PARALLEL_BEAM):
        kw = geometry.scanner_args(scanner, (size, size))
        cone = scanner["mode"] == "cone"
        rays = geometry.scan_rays(torch.tensor([0.6], dtype=torch.float64, device=dev), **kw).float()
        G = torch.rand((1, size, size), device=dev)
        r = {}
        with torch.no_grad():
            r["fwd"] = timed(lambda: project_gaussians_rays(rays, cone, size, size, *leaves), reps, dev)
        rg = rays.clone().requires_grad_(True)
        r["fwd_rays_bwd"] = timed(lambda: torch.autograd.grad(project_gaussians_rays(rg, cone, size, size, *leaves), [rg], G),
                                  reps, dev)
        out[scanner["mode"]] = r
    return out


def recovery(leaves, size, views, iters, lr, dev):
    kw = geometry.scanner_args(S.CONE_BEAM, (size, size))
    g = torch.Generator().manual_seed(11)
    angles = torch.linspace(0.0, 2.0 * np.pi, views + 1, dtype=torch.float64)[:-1].to(dev)
    jitter = 0.01 * torch.randn(views, generator=g, dtype=torch.float64)
    jitter = (jitter - jitter.mean()).to(dev)
    pitch = kw["dDetector"]
    true = {"offDetector": torch.tensor([-1.3 * pitch[0], 2.1 * pitch[1]], dtype=torch.float64, device=dev),
            "roll": torch.tensor(0.02, dtype=torch.float64, device=dev), "d_angle": jitter}
    rays_fn = lambda p: geometry.scan_rays(angles, **dict(kw, offDetector=p["offDetector"], roll=p["roll"], d_angle=p["d_angle"]))
    with torch.no_grad():
        projs = project_gaussians_rays(rays_fn(true), True, size, size, *leaves)
    start = {k: torch.zeros_like(v) for k, v in true.items()}
    got, hist = geometry.refine_geometry(projs, leaves, rays_fn, start, iters, lr)

    def errors(p):
        da = (p["d_angle"] - true["d_angle"])
        return {"offDetector_rows_pixels": float((p["offDetector"][0] - true["offDetector"][0]).abs() / pitch[0]),
                "offDetector_columns_pixels": float((p["offDetector"][1] - true["offDetector"][1]).abs() / pitch[1]),
                "roll_rad": float((p["roll"] - true["roll"]).abs()),
                "d_angle_max_rad": float((da - da.mean()).abs().max()), "d_angle_common_rad": float(da.mean())}

    return {"views": views, "size": size, "iters": iters, "lr": lr, "before": errors(start), "after": errors(got),
            "loss_first": float(hist[0]), "loss_last": float(hist[-1])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--P", type=int, default=50000)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--rec-size", type=int, default=128)
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--lr", type=float, default=2e-3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default="", help="also write the results to this JSON file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("geometry_error.py measures on the GPU: none visible")
    dev = torch.device("cuda:0")
    cloud = S.make_cloud(a.P, seed=7)
    leaves = [t.to(dev) for t in (cloud.xyz, cloud.density, cloud.scales, cloud.rotations)]
    res = {"P": a.P}
    if a.reps:
        res["times_%d" % a.size] = times(leaves, a.size, dev, a.reps)
        print("times", json.dumps(res["times_%d" % a.size]))
        sys.stdout.flush()
    if a.iters:
        res["recovery"] = recovery(leaves, a.rec_size, a.views, a.iters, a.lr, dev)
        print("recovery", json.dumps(res["recovery"]))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
