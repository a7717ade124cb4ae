"""How far is the voxelizer's volume from the density field it samples, and what does the exact query cost?  (DESIGN.md
section 4, "Exact evaluation of the density field".)

    python scripts/field_error.py [--P 50000] [--n 128] [--trained small] [--out field_error.json]

For a scene.make_cloud cloud and, with --trained NAME, a trained cloud (tests/trained_cloud.py, scripts/train_cloud.py): the
voxelizer's volume on an n^3 grid over [-1, 1]^3 against field.query_points at the voxel centres -- max and RMS difference
relative to the exact volume's maximum, and the PSNR between the two (peak = the exact volume's maximum).

Times: one pair of HIP events around every call after a warm-up; the median over `reps` calls with the smallest and the
largest, forward alone (no grad) and forward + backward (all five gradients), for a size^2 oblique plane through the cloud
and a 32^3 patch of voxel centres.  Not a test and not a gate.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from r2_gaussian_amd import GaussianVoxelizationSettings, GaussianVoxelizer   # noqa: E402
from r2_gaussian_amd import scene as S                                        # noqa: E402
from r2_gaussian_amd.field import plane_points, query_points, voxel_centres   # noqa: E402


def compare(a, b):
    """a against the exact b (float64 arrays): max, RMS relative to max(b), PSNR with peak max(b)."""
    d = a - b
    peak = float(b.max())
    mse = float((d * d).mean())
    return {"max_rel": float(np.abs(d).max() / peak), "rms_rel": float(np.sqrt(mse) / peak),
            "psnr": float(10 * np.log10(peak * peak / mse)) if mse > 0 else float("inf")}


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


def time_points(pts, leaves, reps, dev):
    out = {"N": int(pts.numel() // 3)}
    with torch.no_grad():
        out["fwd"] = timed(lambda: query_points(pts, *leaves), reps, dev)
    lg = [t.clone().requires_grad_(True) for t in leaves] + [pts.clone().requires_grad_(True)]
    G = torch.rand(pts.shape[:-1], device=dev)
    out["fwd_bwd"] = timed(lambda: torch.autograd.grad(query_points(lg[4], *lg[:4]), lg, G), max(1, reps // 4), dev)
    return out


def one(cloud, n, size, dev, reps):
    leaves = [t.to(dev) for t in (cloud.xyz, cloud.density, cloud.scales, cloud.rotations)]
    vs = GaussianVoxelizationSettings(1.0, n, n, n, 2.0, 2.0, 2.0, 0.0, 0.0, 0.0, False, False)
    with torch.no_grad():
        vol, _ = GaussianVoxelizer(vs)(leaves[0], leaves[1], scales=leaves[2], rotations=leaves[3])
        exact = query_points(voxel_centres((0.0, 0.0, 0.0), (n, n, n), (2.0, 2.0, 2.0), dev), *leaves)
    out = {"P": int(cloud.xyz.shape[0]), "n": n, "voxelizer_vs_exact": compare(vol.double().cpu().numpy(), exact.double().cpu().numpy())}
    if reps:
        with torch.no_grad():
            out["exact_volume_fwd"] = timed(lambda: query_points(voxel_centres((0.0, 0.0, 0.0), (n, n, n), (2.0, 2.0, 2.0), dev), *leaves),
                                            max(1, reps // 4), dev)
        d = 1.8 / size   # an oblique plane through the origin, inside the cube
        u = np.array([0.8, 0.5, 0.33]) / np.linalg.norm([0.8, 0.5, 0.33]) * d
        v = np.cross([0.2, -0.7, 0.68], u)
        v = v / np.linalg.norm(v) * d
        plane = plane_points(-(u + v) * size / 2, u, v, size, size, dev)
        out["plane_%d" % size] = time_points(plane, leaves, reps, dev)
        out["patch_32"] = time_points(voxel_centres((0.1, -0.1, 0.0), (32, 32, 32), (0.25, 0.25, 0.25), dev), leaves, reps, dev)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--P", type=int, default=50000)
    ap.add_argument("--n", type=int, default=128)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--trained", default="")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default="", help="also write the results to this JSON file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("field_error.py measures on the GPU: none visible")
    dev = torch.device("cuda:0")
    res = {}
    clouds = [("make_cloud", S.make_cloud(a.P, seed=7))]
    if a.trained:
        from tests import trained_cloud
        c, _info = trained_cloud.load(a.trained)
        clouds.append(("trained_" + a.trained, c))
    for name, cloud in clouds:
        res[name] = r = one(cloud, a.n, a.size, dev, a.reps)
        print(name, json.dumps(r))
        sys.stdout.flush()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
