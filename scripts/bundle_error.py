"""What do exact line integrals along arbitrary rays cost, next to the projector that takes whole flat detectors?
("Line integrals along arbitrary rays".)

    python scripts/bundle_error.py [--P 50000] [--size 512] [--views 50] [--reps 20] [--out bundle_error.json]

Times: one pair of HIP events around every call after a warm-up; the median over `reps` calls with the smallest and the
largest, for a scene.make_cloud cloud of P Gaussians: the forward alone, forward + parameter backward (only the four
parameter tensors require grad) and forward + ray backward (only the rays do).
  (a) the size^2 pixels of one cone view in the order of 16 x 16 tiles, next to project_gaussians_rays on the same view, and
      the largest difference between the two images relative to the image's maximum;
  (b) 4096 and 65 536 random pixels over `views` views, as drawn and with sort=True;
  (c) a 512 x 64 curved detector (64 rows of 512 columns on the arc of the flat detector's width), one view.
Under every row the same rays with method="leaves" (culling by leaves of 64 Gaussians), in the same process by the same
protocol; on (b) also with order=True (the gathers by cloud_order inside the timing) and with the cloud put into
cloud_order once, outside the timing.
Not a test and not a gate.
"""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from r2_gaussian_amd import geometry                                                          # noqa: E402
from r2_gaussian_amd import scene as S                                                        # noqa: E402
from r2_gaussian_amd.gaussian_projector import cloud_order, integrate_rays, project_gaussians_rays   # noqa: E402


def timed(fn, reps, dev, warm=3):
    """-> dict(median_ms, min_ms, max_ms, reps, warm): every call between its own pair of events."""
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
    return {"median_ms": t[len(t) // 2], "min_ms": t[0], "max_ms": t[-1], "reps": reps, "warm": warm}


def three(o, d, leaves, half_line, sort, reps, dev, method="blocks", order=False):
    """Forward, forward + parameter backward, forward + ray backward of integrate_rays on the rays (o, d)."""
    G = torch.rand(o.shape[:-1], device=dev)
    call = lambda o, d, lv: integrate_rays(o, d, *lv, half_line=half_line, sort=sort, method=method, order=order)
    r = {"rays": int(G.numel())}
    with torch.no_grad():
        r["fwd"] = timed(lambda: call(o, d, leaves), reps, dev)
    lg = [t.clone().requires_grad_(True) for t in leaves]
    r["fwd_param_bwd"] = timed(lambda: torch.autograd.grad(call(o, d, lg), lg, G), reps, dev)
    og, dg = o.clone().requires_grad_(True), d.clone().requires_grad_(True)
    r["fwd_rays_bwd"] = timed(lambda: torch.autograd.grad(call(og, dg, leaves), [og, dg], G), reps, dev)
    return r


def tile_order(H, W, dev, tile=16):
    """rows, cols [1, H * W]: the pixels of the detector tile by tile (row-major tiles, row-major inside a tile)."""
    r, c = torch.meshgrid(torch.arange(H, device=dev), torch.arange(W, device=dev), indexing="ij")
    key = ((r // tile) * ((W + tile - 1) // tile) + c // tile) * (tile * tile) + (r % tile) * tile + c % tile
    order = torch.argsort(key.reshape(-1))
    return r.reshape(-1)[order][None], c.reshape(-1)[order][None]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--P", type=int, default=50000)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--views", type=int, default=50)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default="", help="also write the results to this JSON file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bundle_error.py measures on the GPU: none visible")
    dev = torch.device("cuda:0")
    cloud = S.make_cloud(a.P, seed=7)
    leaves = [t.to(dev) for t in (cloud.xyz, cloud.density, cloud.scales, cloud.rotations)]
    n = a.size
    kw = geometry.scanner_args(S.CONE_BEAM, (n, n))
    res = {"P": a.P, "size": n}

    def emit(key, val):
        res[key] = val
        print(key, json.dumps(val))
        sys.stdout.flush()

    # (a) one cone view, tile order, against the projector
    rays = geometry.scan_rays(torch.tensor([0.6], dtype=torch.float64, device=dev), **kw).float()
    rows, cols = tile_order(n, n, dev)
    o, d = geometry.pixel_rays(rays, True, n, n, rows, cols)
    one = three(o, d, leaves, True, False, a.reps, dev)
    proj = {}
    G = torch.rand((1, n, n), device=dev)
    with torch.no_grad():
        proj["fwd"] = timed(lambda: project_gaussians_rays(rays, True, n, n, *leaves), a.reps, dev)
        img = project_gaussians_rays(rays, True, n, n, *leaves)
        mine = torch.zeros_like(img)
        mine[0, rows[0], cols[0]] = integrate_rays(o, d, *leaves, half_line=True)[0]
    lg = [t.clone().requires_grad_(True) for t in leaves]
    proj["fwd_param_bwd"] = timed(lambda: torch.autograd.grad(project_gaussians_rays(rays, True, n, n, *lg), lg, G), a.reps, dev)
    rg = rays.clone().requires_grad_(True)
    proj["fwd_rays_bwd"] = timed(lambda: torch.autograd.grad(project_gaussians_rays(rg, True, n, n, *leaves), [rg], G), a.reps, dev)
    emit("a_view_tile_order", one)
    emit("a_view_tile_order_leaves", three(o, d, leaves, True, False, a.reps, dev, method="leaves"))
    emit("a_projector", proj)
    emit("a_max_difference_over_image_max", float((mine - img).abs().max() / img.abs().max()))

    # (b) random pixels over many views
    angles = torch.linspace(0.0, 2.0 * math.pi, a.views + 1, dtype=torch.float64, device=dev)[:-1]
    many = geometry.scan_rays(angles, **kw).float()
    g = torch.Generator(device="cpu").manual_seed(3)
    perm = cloud_order(leaves[0], leaves[2])
    ordered = [t[perm].contiguous() for t in leaves]   # the cloud put into cloud_order once, outside the timing
    for total in (4096, 65536):
        k = total // a.views
        rows = torch.randint(n, (a.views, k), generator=g).to(dev)
        cols = torch.randint(n, (a.views, k), generator=g).to(dev)
        o, d = geometry.pixel_rays(many, True, n, n, rows, cols)
        mix = torch.randperm(a.views * k, generator=g).to(dev)   # drawn across the views, not view by view
        o, d = o.reshape(-1, 3)[mix].contiguous(), d.reshape(-1, 3)[mix].contiguous()
        for sort in (False, True):
            key = "b_random_%d%s" % (total, "_sorted" if sort else "")
            emit(key, three(o, d, leaves, True, sort, a.reps, dev))
            emit(key + "_leaves", three(o, d, leaves, True, sort, a.reps, dev, method="leaves"))
        emit("b_random_%d_leaves_order" % total, three(o, d, leaves, True, False, a.reps, dev, method="leaves", order=True))
        emit("b_random_%d_leaves_preordered" % total, three(o, d, ordered, True, False, a.reps, dev, method="leaves"))

    # (c) a curved detector: 64 rows of 512 columns, the arc as long as the flat detector is wide
    W, H = 512, 64
    width = kw["dDetector"][1] * n
    o, d = geometry.curved_detector_rays(torch.tensor([0.6], dtype=torch.float64, device=dev), kw["DSO"], kw["DSD"],
                                         width / kw["DSD"] / W, kw["dDetector"][0] * n / H, (H, W))
    o, d = o.float().contiguous(), d.float().contiguous()
    emit("c_curved_512x64", three(o, d, leaves, True, False, a.reps, dev))
    emit("c_curved_512x64_leaves", three(o, d, leaves, True, False, a.reps, dev, method="leaves"))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
