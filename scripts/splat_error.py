"""How far is the splatting rasterizer's image from the true line integrals of the model?  ("Exact
projection of the Gaussian model".)

    python scripts/splat_error.py [--P 50000] [--size 512] [--trained small] [--out splat_error.json]

For a scene.make_cloud cloud and, with --trained NAME, a trained cloud (tests/trained_cloud.py, scripts/train_cloud.py), in
cone and parallel beam: the rasterizer's image against gaussian_projector.project_gaussians -- max and RMS difference
relative to the image maximum, and the PSNR between the two (peak = the exact image's maximum).

The split of the difference needs the exact projection cut at q <= 9, which the kernel does not offer: it is taken on the
host, from the float64 restatement (tests/gaussian_project_ref.py, qmax = 9 against qmax = None), on a problem small enough
for it (--host_P Gaussians, --host_size^2 pixels, the same cloud recipe).  exact - exact(q <= 9) is what the cut explains;
the rest of raster - exact is the affine approximation (cone beam; in parallel beam splatting is exact up to its cut, and
the rest is the cut's square against the ellipse q = 9).

Times: HIP events around `reps` back-to-back calls after a warm-up, forward alone and forward + backward, per view.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from r2_gaussian_amd import GaussianRasterizationSettings, GaussianRasterizer   # noqa: E402
from r2_gaussian_amd import scene as S                                            # noqa: E402
from r2_gaussian_amd.gaussian_projector import project_gaussians, world_ray_params   # noqa: E402


def raster(v, leaves, dev):
    rs = GaussianRasterizationSettings(v.image_height, v.image_width, v.tanfovx, v.tanfovy, 1.0, v.world_view_transform.to(dev),
                                       v.full_proj_transform.to(dev), v.camera_center.to(dev), False, v.mode, False)
    img, _ = GaussianRasterizer(rs)(leaves[0], torch.zeros_like(leaves[0]), leaves[1], scales=leaves[2], rotations=leaves[3])
    return img.reshape(v.image_height, v.image_width)


def compare(a, b):
    """a against the exact b (float64 arrays): max, RMS relative to max(b), PSNR with peak max(b)."""
    d = a - b
    peak = float(b.max())
    mse = float((d * d).mean())
    return {"max_rel": float(np.abs(d).max() / peak), "rms_rel": float(np.sqrt(mse) / peak),
            "psnr": float(10 * np.log10(peak * peak / mse)) if mse > 0 else float("inf")}


def timed(fn, reps, dev):
    for _ in range(3):
        fn()
    torch.cuda.synchronize(dev)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize(dev)
    return a.elapsed_time(b) / reps


def one(cloud, beam, size, dev, reps, host=None):
    cfg = S.CONE_BEAM if beam == "cone" else S.PARALLEL_BEAM
    v = S.make_view(0.6, (size, size), cfg)
    leaves = [t.to(dev) for t in (cloud.xyz, cloud.density, cloud.scales, cloud.rotations)]
    with torch.no_grad():
        ex = project_gaussians([v], *leaves)[0]
        ra = raster(v, leaves, dev)
    out = {"P": int(cloud.xyz.shape[0]), "size": size, "raster_vs_exact": compare(ra.double().cpu().numpy(), ex.double().cpu().numpy())}
    if reps:
        with torch.no_grad():
            out["exact_fwd_ms"] = timed(lambda: project_gaussians([v], *leaves), reps, dev)
            out["raster_fwd_ms"] = timed(lambda: raster(v, leaves, dev), reps, dev)
        G = torch.rand((1, size, size), device=dev)
        lg = [t.clone().requires_grad_(True) for t in leaves]

        def fb():
            for t in lg:
                t.grad = None
            (project_gaussians([v], *lg) * G).sum().backward()
        out["exact_fwd_bwd_ms"] = timed(fb, max(1, reps // 4), dev)
    if host is not None:
        from tests import gaussian_project_ref as R
        hc, hsize = host
        hv = S.make_view(0.6, (hsize, hsize), cfg)
        hl = [t.to(dev) for t in (hc.xyz, hc.density, hc.scales, hc.rotations)]
        with torch.no_grad():
            hra = raster(hv, hl, dev).double().cpu().numpy()
            hex_ = project_gaussians([hv], *hl)[0].double().cpu().numpy()
        args = (world_ray_params([hv]), beam == "cone", hsize, hsize, hc.xyz.numpy(), hc.density.numpy(), hc.scales.numpy(),
                hc.rotations.numpy())
        full, cut = R.project64(*args)["img"][0], R.project64(*args, qmax=9.0)["img"][0]
        out["host"] = {"P": int(hc.xyz.shape[0]), "size": hsize, "kernel_vs_float64": compare(hex_, full),
                       "raster_vs_exact": compare(hra, full), "cut_q9_vs_exact": compare(cut, full),
                       "raster_vs_cut_q9": compare(hra, cut)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--P", type=int, default=50000)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--host_P", type=int, default=2000)
    ap.add_argument("--host_size", type=int, default=128)
    ap.add_argument("--trained", default="")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default="", help="also write the results to this JSON file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("splat_error.py measures on the GPU: none visible")
    dev = torch.device("cuda:0")
    res = {}
    clouds = [("make_cloud", S.make_cloud(a.P, seed=7), (S.make_cloud(a.host_P, seed=7), a.host_size))]
    if a.trained:
        from tests import trained_cloud
        c, _info = trained_cloud.load(a.trained)
        clouds.append(("trained_" + a.trained, c, None))
    for name, cloud, host in clouds:
        for beam in ("cone", "parallel"):
            res[name + "/" + beam] = r = one(cloud, beam, a.size, dev, a.reps, host)
            print(name, beam, json.dumps(r))
            sys.stdout.flush()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
