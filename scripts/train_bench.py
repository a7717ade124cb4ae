#!/usr/bin/env python
"""Whole training iterations at the headline workload, three model / optimizer variants on the same kernels:

    python scripts/train_bench.py [--P 300000] [--iters 200] [--warmup 30] [--rounds 3] [--profile DIR]

  foreach   tests/mini_trainer.Model: torch activations + autograd, torch.optim.Adam (foreach, the default on the device)
  fused     the same with torch.optim.Adam(fused=True)
  native    r2_gaussian_amd.gaussians.GaussianModel: one r2_gaussian_adam_step launch (activation backward, Adam, next
            activations)

An iteration: render one 512^2 cone-beam view (cycling over 8), fused L1 + D-SSIM loss against a fixed target, a 32^3 TV patch
through the voxelizer and the fused TV loss, backward, the fused densification statistics, the model step.  No densify
steps.  All variants start from the same seeded 300k-Gaussian cloud; they run alternating, `--rounds` timed windows of
`--iters` iterations each after `--warmup` untimed ones, timed with a host clock between device synchronisations.  Prints one
JSON line: it/s per variant (median over the rounds, and all rounds).

--views [W ...] (default 2 4 8) measures several views per optimiser step instead, on the native model: whole steps of W
views through one GaussianRasterizerBatch call followed by
  loop     a per-view loop of losses.image_loss and densify.densification_stats (2 W + W launches, W autograd nodes), or
  batched  losses.image_loss_batch and densify.densification_stats_batch (2 launches per 16 views + 1, one node),
the rest of the step the same (one TV patch, one backward, one model step); W = 1 through the single-view calls for scale.
All legs alternate round by round in one process; steps/s and views/s per leg, median over the rounds, and the spread.
With --profile DIR: a separate run of the batched leg at the largest W under ``rocprofv3 --kernel-trace --stats`` and the
mean times of the two batched loss kernels and the batched statistics kernel.

--profile DIR: in addition, a separate run of the native variant alone under
``rocprofv3 --kernel-trace --stats`` (output under DIR), and the step kernel's mean time against its HBM byte floor:
340 B per Gaussian (read params, grads, exp_avg, exp_avg_sq: 44 floats; write params and both moments: 33 floats, and the
next activations: 8 floats) over 6.3 TB/s (the achievable HBM rate of MI355X_MICROARCH.md).
"""
import argparse
import csv
import glob
import json
import os
import statistics
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_ACHIEVABLE_GBS = 6300.0
STEP_BYTES_PER_GAUSSIAN = 4 * (44 + 33 + 8)
STEP_KERNEL = "gaussian_adam_kernel"


def make_variants(P, names):
    from tests import mini_trainer as T
    from r2_gaussian_amd import scene as S
    from r2_gaussian_amd.gaussians import GaussianModel
    from r2_gaussian_amd.train import OptimizationParams
    dev = torch.device("cuda:0")
    cloud = S.make_cloud(P, seed=0)
    init_density = cloud.density.reshape(-1)
    lo, hi = T.Opt.scale_min * 2.0, T.Opt.scale_max * 2.0
    native = GaussianModel((lo, hi), device=dev)
    native.create_from_pcd(cloud.xyz.numpy(), init_density[:, None].numpy(), 1.0)
    native.training_setup(OptimizationParams())
    out = {}
    for name in names:
        if name == "native":
            out[name] = native
            continue
        opt = T.Opt(iterations=30000)
        m = T.Model.from_tensors(opt, T.Backend("hip"), {n: native._raw[n].detach() for n in T.Model.NAMES})
        if name == "fused":
            m.optimizer = torch.optim.Adam([{"params": [m.p[n]], "lr": m.lr[n](0), "name": n} for n in m.NAMES], lr=0.0,
                                           eps=1e-15, fused=True)
        out[name] = m
    return out


def make_iteration(model, views, gts, tvN, tvS):
    from r2_gaussian_amd import densify as FD
    from r2_gaussian_amd import losses as FL
    from r2_gaussian_amd.gaussians import GaussianModel
    from r2_gaussian_amd.train import _query, _settings
    from r2_gaussian_amd import GaussianRasterizer
    dev = torch.device("cuda:0")
    settings = [_settings(v, dev) for v in views]
    centre = torch.zeros(3)
    native = isinstance(model, GaussianModel)

    def iteration(it):
        if native:
            x, d, s, r = model.activated()
        else:
            model.update_lr(it)
            x, d, s, r = model.activated()
        screen = torch.zeros_like(x, requires_grad=True)
        img, radii = GaussianRasterizer(settings[it % len(views)])(x, screen, d, scales=s, rotations=r)
        loss, _ = FL.image_loss(img, gts[it % len(views)], 0.25)
        loss = loss + 0.05 * FL.tv_3d_loss(_query(x, d, s, r, centre, tvN, tvS))
        loss.backward()
        with torch.no_grad():
            if native:
                model.add_densification_stats(radii, screen.grad)
                model.step(it)
            else:
                FD.densification_stats(radii, screen.grad, model.max_radii2D, model.grad_accum, model.denom)
                model.optimizer.step()
                model.optimizer.zero_grad(set_to_none=True)
    return iteration


def make_views_step(model, views, gts, tvN, tvS, W, batched):
    """One optimiser step of the native model on W views (cycling over the 8 views in blocks of W)."""
    from r2_gaussian_amd import densify as FD
    from r2_gaussian_amd import losses as FL
    from r2_gaussian_amd import GaussianRasterizerBatch
    from r2_gaussian_amd.train import _query, _settings
    dev = torch.device("cuda:0")
    blocks = [[(b * W + k) % len(views) for k in range(W)] for b in range(max(1, len(views) // W))]
    settings = [_settings(views[blk[0]], dev, [views[i] for i in blk]) for blk in blocks]
    centre = torch.zeros(3)

    def step(it):
        blk = blocks[it % len(blocks)]
        x, d, s, r = model.activated()
        screen = torch.zeros((W,) + tuple(x.shape), dtype=torch.float32, device=dev, requires_grad=True)
        imgs, radii = GaussianRasterizerBatch(settings[it % len(blocks)])(x, screen, d, scales=s, rotations=r)
        if batched:
            loss, _ = FL.image_loss_batch(imgs, [gts[i] for i in blk], 0.25)
        else:
            loss = 0.0
            for v, i in enumerate(blk):
                loss = loss + FL.image_loss(imgs[v:v + 1], gts[i], 0.25)[0]
            loss = loss * (1.0 / W)
        loss = loss + 0.05 * FL.tv_3d_loss(_query(x, d, s, r, centre, tvN, tvS))
        loss.backward()
        with torch.no_grad():
            if batched:
                model.add_densification_stats(radii, screen.grad, grad_scale=float(W))
            else:
                for v in range(W):
                    FD.densification_stats(radii[v], screen.grad[v], model.max_radii2D, model.xyz_gradient_accum, model.denom)
            model.step(it)
    return step


def run_views(args):
    """-> {leg: [steps/s per round]} for the legs w1, loop_W, batched_W."""
    from r2_gaussian_amd import scene as S
    views = S.make_views(8, (512, 512))
    g = torch.Generator().manual_seed(1)
    gts = [torch.rand((1, 512, 512), generator=g).cuda() * 0.5 for _ in views]
    tvN = torch.tensor([32, 32, 32])
    tvS = torch.tensor([2.0 / 256] * 3) * tvN
    legs = {}
    if not args.only_batched:
        legs["w1"] = (1, make_iteration(make_variants(args.P, ["native"])["native"], views, gts, tvN, tvS))
    for W in args.views:
        for name, batched in (("loop", False), ("batched", True)):
            if args.only_batched and not batched:
                continue
            model = make_variants(args.P, ["native"])["native"]
            legs["%s_%d" % (name, W)] = (W, make_views_step(model, views, gts, tvN, tvS, W, batched))
    counters = {n: 1 for n in legs}
    for n, (_W, step) in legs.items():
        for _ in range(args.warmup):
            step(counters[n])
            counters[n] += 1
    torch.cuda.synchronize()
    rates = {n: [] for n in legs}
    for _ in range(args.rounds):
        for n, (W, step) in legs.items():
            iters = max(10, args.iters // W)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(iters):
                step(counters[n])
                counters[n] += 1
            torch.cuda.synchronize()
            rates[n].append(iters / (time.perf_counter() - t0))
    return {n: (legs[n][0], v) for n, v in rates.items()}


VIEW_KERNELS = ("ssim_forward_kernel", "ssim_backward_kernel", "densify_stats_batch_kernel")


def profile_views(args):
    d = os.path.abspath(args.profile)
    os.makedirs(d, exist_ok=True)
    W = max(args.views)
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "train_bench_views", "--",
           sys.executable, os.path.abspath(__file__), "--P", str(args.P), "--iters", str(20 * W), "--warmup", "5", "--rounds", "1",
           "--views", str(W), "--only-batched"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        raise RuntimeError("rocprofv3 run failed:\n" + r.stdout[-2000:] + r.stderr[-4000:])
    files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        raise RuntimeError("no kernel_stats.csv under " + d)
    out = {"W": W}
    for row in csv.DictReader(open(files[0])):
        for k in VIEW_KERNELS:
            if k in row["Name"]:
                out[k] = {"calls": int(row["Calls"]), "avg_us": float(row["AverageNs"]) / 1e3,
                          "percent": float(row["Percentage"])}
    missing = [k for k in VIEW_KERNELS if k not in out]
    if missing:
        raise RuntimeError("%s not in %s" % (missing, files[0]))
    return out


def run(args, names):
    from r2_gaussian_amd import scene as S
    views = S.make_views(8, (512, 512))
    g = torch.Generator().manual_seed(1)
    gts = [torch.rand((1, 512, 512), generator=g).cuda() * 0.5 for _ in views]
    tvN = torch.tensor([32, 32, 32])
    tvS = torch.tensor([2.0 / 256] * 3) * tvN
    models = make_variants(args.P, names)
    its = {n: make_iteration(models[n], views, gts, tvN, tvS) for n in names}
    counters = {n: 1 for n in names}
    for n in names:
        for _ in range(args.warmup):
            its[n](counters[n])
            counters[n] += 1
    torch.cuda.synchronize()
    rates = {n: [] for n in names}
    for _ in range(args.rounds):
        for n in names:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.iters):
                its[n](counters[n])
                counters[n] += 1
            torch.cuda.synchronize()
            rates[n].append(args.iters / (time.perf_counter() - t0))
    return rates


def profile(args):
    d = os.path.abspath(args.profile)
    os.makedirs(d, exist_ok=True)
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "train_bench", "--",
           sys.executable, os.path.abspath(__file__), "--P", str(args.P), "--iters", "50", "--warmup", "5", "--rounds", "1",
           "--only", "native"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        raise RuntimeError("rocprofv3 run failed:\n" + r.stdout[-2000:] + r.stderr[-4000:])
    files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        raise RuntimeError("no kernel_stats.csv under " + d)
    rows = [row for row in csv.DictReader(open(files[0])) if STEP_KERNEL in row["Name"]]
    if not rows:
        raise RuntimeError("%s not in %s" % (STEP_KERNEL, files[0]))
    us = float(rows[0]["AverageNs"]) / 1e3
    floor_us = args.P * STEP_BYTES_PER_GAUSSIAN / (HBM_ACHIEVABLE_GBS * 1e3)
    return {"kernel": rows[0]["Name"], "calls": int(rows[0]["Calls"]), "avg_us": us, "byte_floor_us": floor_us,
            "floor_fraction": floor_us / us, "bytes": args.P * STEP_BYTES_PER_GAUSSIAN}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--P", type=int, default=300_000)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--only", choices=["foreach", "fused", "native"], default=None)
    ap.add_argument("--profile", default=None, help="directory for the rocprofv3 run of the native variant")
    ap.add_argument("--views", type=int, nargs="*", default=None, metavar="W",
                    help="measure steps of W views each (default 2 4 8): per-view loss / statistics loop against the batched calls")
    ap.add_argument("--only-batched", action="store_true", help="with --views: the batched leg alone (what --profile runs)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "train_bench.py measures on the GPU"
    if args.views is not None:
        args.views = args.views or [2, 4, 8]
        if min(args.views) < 2 or max(args.views) > 8:
            ap.error("--views: 2 <= W <= 8 (the leg cycles over 8 views)")
        rates = run_views(args)
        out = {"P": args.P, "detector": 512, "tv_patch": 32, "iters_per_round": args.iters, "rounds": args.rounds, "legs": {
            n: {"W": W, "steps_per_s": statistics.median(v), "views_per_s": W * statistics.median(v),
                "spread": (max(v) - min(v)) / statistics.median(v), "steps_per_s_rounds": v} for n, (W, v) in rates.items()}}
        # the models train while they are timed, so every leg's rate drifts with its cloud; the two legs of one W have taken
        # the same number of steps when a round starts, which makes the ratio round by round the comparison to read
        out["batched_over_loop"] = {}
        for W in args.views:
            if "loop_%d" % W in rates and "batched_%d" % W in rates:
                q = [b / a for a, b in zip(rates["loop_%d" % W][1], rates["batched_%d" % W][1])]
                out["batched_over_loop"][W] = {"median": statistics.median(q), "min": min(q), "max": max(q)}
        if args.profile and not args.only_batched:
            out["kernels"] = profile_views(args)
        print(json.dumps(out))
        return
    names = [args.only] if args.only else ["foreach", "fused", "native"]
    rates = run(args, names)
    out = {"P": args.P, "detector": 512, "tv_patch": 32, "iters_per_round": args.iters, "rounds": args.rounds,
           "it_per_s": {n: statistics.median(v) for n, v in rates.items()}, "it_per_s_rounds": rates}
    if args.profile and not args.only:
        out["step_kernel"] = profile(args)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
