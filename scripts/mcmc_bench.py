"""What do the position noise and the relocation cost, and what does the fixed-budget strategy do to a short training run?
("Relocation and position noise".)

    python scripts/mcmc_bench.py [--P 50000 300000] [--reps 20] [--iterations 1500] [--out mcmc_bench.json]

On scene.make_cloud clouds, in one process:

* times of ``mcmc.position_noise`` (one launch), of ``mcmc.relocate`` (plan + emit, no host read; 30 % of the rows dead, 5 %
  appended) and of ``densify.densify_and_prune`` (classify + emit, one host read; the threshold set so that about 30 % of the
  rows are cloned or split) on the same cloud with Adam moments and statistics;
* a training run of `--iterations` on a 64^3 phantom written by datagen (128^2 detector, 50 views) with the threshold strategy
  and with ``--densify_strategy mcmc`` capped at the count the threshold run ended with: 3D PSNR / SSIM and P of each.

Times: one pair of HIP events around every call after three warm-up calls, the median over `reps` calls with the smallest and
the largest (scripts/field_error.timed).  One process, one run.  Reports, and promises nothing: not a test and not a gate.  The
strategy's numbers (noise_lr, its density and sharpness, dead_density, the two L1 weights) are the original method's, untuned
for CT.
"""
import argparse
import json
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from r2_gaussian_amd import densify as D                                                     # noqa: E402
from r2_gaussian_amd import mcmc as MC                                                       # noqa: E402
from r2_gaussian_amd import scene as S                                                       # noqa: E402
from r2_gaussian_amd.gaussians import NAMES, activate                                        # noqa: E402
from scripts.field_error import timed                                                        # noqa: E402


def bench_cloud(P, reps, dev, emit):
    c = S.make_cloud(P, seed=7)
    g = torch.Generator().manual_seed(P)
    dens = c.density.clone()
    dens[torch.rand(P, generator=g) < 0.3] = 1e-3                     # 30 % dead at dead_density 0.005
    raw = {"xyz": c.xyz, "density": torch.log(torch.expm1(dens)), "scaling": torch.log(c.scales), "rotation": c.rotations}
    raw = {n: raw[n].to(dev).float().contiguous() for n in NAMES}
    moments = {n: (torch.randn_like(raw[n]), torch.rand_like(raw[n])) for n in NAMES}
    stats = (torch.rand(P, device=dev) * 10, torch.rand(P, device=dev), torch.rand(P, device=dev) + 1)
    act = activate(raw["density"], raw["scaling"], raw["rotation"], None)
    xyz = raw["xyz"].clone()
    n_new = P // 20
    normals = torch.randn((2, P, 3), generator=g).to(dev)
    bbox = torch.tensor([[-2.0, -2.0, -2.0], [2.0, 2.0, 2.0]])
    thr = float(torch.quantile((stats[1] / stats[2])[:: max(1, P // 100000)], 0.7))
    dp = lambda: D.densify_and_prune(raw, moments, stats[0], stats[1], stats[2], normals, thr, 0.05, 1e-5, bbox)
    counts = dp()[5]
    info = MC.relocate(raw, moments, stats, 0.005, n_new=n_new, call=1, counts=True, activated=act)[3]
    emit("time_P%dk" % (P // 1000), {
        "P": P, "dead": info["dead"], "n_new": n_new, "densify_counts": list(counts),
        "position_noise": timed(lambda: MC.position_noise(xyz, *act, 100.0, call=1), reps, dev),
        "relocate_plan_emit": timed(lambda: MC.relocate(raw, moments, stats, 0.005, n_new=n_new, call=1, activated=act), reps, dev),
        "relocate_with_activation": timed(lambda: MC.relocate(raw, moments, stats, 0.005, n_new=n_new, call=1), reps, dev),
        "densify_and_prune": timed(dp, reps, dev)})


def _blob(n, c0, sigma, rho):
    ax = -1 + (np.arange(n) + 0.5) * 2.0 / n
    X, Y, Z = np.meshgrid(ax, ax, ax, indexing="ij")
    return (rho * np.exp(-((X - c0[0]) ** 2 + (Y - c0[1]) ** 2 + (Z - c0[2]) ** 2) / (2 * sigma ** 2))).astype(np.float32)


def bench_training(iterations, emit):
    from r2_gaussian_amd import datagen
    from r2_gaussian_amd import train as TR
    n = 64
    vol = _blob(n, (0.1, -0.2, 0.05), 0.3, 0.6) + _blob(n, (-0.3, 0.25, -0.1), 0.12, 0.5) + _blob(n, (0.35, 0.3, 0.2), 0.08, 0.4)
    cfg = dict(S.CONE_BEAM, nVoxel=[n, n, n], nDetector=[128, 128], noise=False, totalAngle=360.0, startAngle=0.0)
    with tempfile.TemporaryDirectory() as tmp:
        case = TR.load_case(datagen.generate(vol, cfg, os.path.join(tmp, "data"), "phantom", n_train=50, n_test=20, seed=0))
        bound = np.array([0.0005, 0.5]) * max(case["geometry"]["sVoxel"])
        window = dict(iterations=iterations, position_lr_max_steps=iterations, density_lr_max_steps=iterations,
                      scaling_lr_max_steps=iterations, rotation_lr_max_steps=iterations, densify_from_iter=iterations // 10,
                      densify_until_iter=iterations - iterations // 10, densification_interval=max(1, iterations // 15))
        cap = None
        for name, extra in (("threshold", {}), ("mcmc", {"densify_strategy": "mcmc"})):
            if name == "mcmc":
                extra["cap_max"] = cap
            opt = TR.OptimizationParams(**window, **extra)
            out = TR.training(case["train_views"], case["train_projs"], case["test_views"], case["test_projs"], case["vol_gt"],
                              case["geometry"], case["init_points"], opt, os.path.join(tmp, name), bound,
                              test_iterations={0, iterations}, log=lambda *a: None)
            cap = out["P"] if cap is None else cap
            emit("train_%s" % name, {"iterations": iterations, "P_init": int(case["init_points"].shape[0]), "P": out["P"],
                                     "cap_max": extra.get("cap_max"), "relocations": out["relocations"],
                                     "psnr_3d_start": out["evals"][0]["psnr_3d"], "psnr_3d": out["evals"][iterations]["psnr_3d"],
                                     "ssim_3d": out["evals"][iterations]["ssim_3d"], "it_per_s": out["it_per_s"],
                                     "window": {k: window[k] for k in ("densify_from_iter", "densify_until_iter",
                                                                        "densification_interval")}})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--P", type=int, nargs="*", default=[50000, 300000])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--iterations", type=int, default=1500, help="training run length (0 = no training run)")
    ap.add_argument("--out", default="", help="also write the results to this JSON file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mcmc_bench.py measures on the GPU: none visible")
    dev = torch.device("cuda:0")
    res = {}

    def emit(key, value):
        res[key] = value
        print(key, json.dumps(value))
        sys.stdout.flush()
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                json.dump(res, f, indent=1)

    for P in a.P:
        bench_cloud(P, a.reps, dev, emit)
    if a.iterations > 0:
        bench_training(a.iterations, emit)


if __name__ == "__main__":
    main()
