"""Timing of the exact adjoint (csrc/backprojector.hip), the TV descent (csrc/tv_descent.hip) and the iterative
reconstructions (r2_gaussian_amd/recon.py) on the MI355X; prints one JSON line.

    python scripts/recon_bench.py [--reps 7] [--warmup 1] [--run-reps 7] [--projection_type interpolated|siddon]

Cases, 256^3 <- 50 x 512^2 at accuracy 0.5 with the reference scanner (tests/golden/scanner/cone_beam.yml):

* backproject_{cone,parallel}: one A^T call over the 50 views, median of --reps after --warmup (HIP events);
* tv_step: one r2_tv_descent iteration at 256^3;
* cgls_iter: one CGLS iteration, the median of cgls(2) minus the median of cgls(1) (A, A^T and the vector updates);
* cgls60, sart20, asd_pocs10: whole runs as ct_utils.py calls them, median of --run-reps.

Beside the adjoint's time, floor_ms is a MODEL, not a measurement: the VALU bound of the work the gather cannot avoid.
Every sample the forward takes carries weight to the 8 corners of its cell, and the gather evaluates it once per corner
voxel: samples x 8 x VALU_PER_VOXEL_SAMPLE wave64 instructions (counted from the sample loop's ISA), one wave64 instruction
per cycle per CU (4 SIMD16s, 4 cycles each), 256 CUs at 2.4 GHz.  The pixel box, the filter and the ray set-ups are
overhead above that floor.  samples: the forward's sample count (scripts/project_bench.py, float64 clip).

With --projection_type siddon the same cases run on the Siddon pair (csrc/projector_siddon.hip, backprojector_siddon.hip), the
interpolated adjoint and forward are timed beside it in the same run (interpolated_ms, interpolated_forward_ms), and the floor
model is the work the gather cannot avoid under that model: one ray set-up and entry (SIDDON_VALU_PER_ENTRY wave64 VALU
instructions, counted from the pixel loop's ISA past the filter) for every (voxel, ray) pair with a non-zero entry, which are
the forward's segments (scripts/project_bench.py: count_segments).  The pixels the box holds and the filter drops are overhead
above that floor.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from r2_gaussian_amd import projector as K   # noqa: E402
from r2_gaussian_amd import recon as RC      # noqa: E402
from r2_gaussian_amd import scene as S       # noqa: E402
from project_bench import count_samples, count_segments      # noqa: E402

CUS, CLOCK = 256, 2.4e9
VALU_PER_VOXEL_SAMPLE = 69.0   # VALU instructions per iteration of backproject_kernel's sample loop (gfx950 ISA)
SIDDON_VALU_PER_ENTRY = 160.0  # VALU instructions of backproject_siddon_kernel's pixel loop body past the filter (gfx950 ISA)


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def phantom(n, dev):
    ax = torch.linspace(-1 + 1.0 / n, 1 - 1.0 / n, n, device=dev)
    X, Y, Z = torch.meshgrid(ax, ax, ax, indexing="ij")
    return (0.6 * torch.exp(-((X - 0.1) ** 2 + (Y + 0.2) ** 2 + Z ** 2) / 0.18)
            + 0.5 * torch.exp(-((X + 0.3) ** 2 + (Y - 0.25) ** 2 + (Z + 0.1) ** 2) / 0.03)).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--run-reps", type=int, default=7)
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--det", type=int, default=512)
    ap.add_argument("--views", type=int, default=50)
    ap.add_argument("--projection_type", default="interpolated", choices=K.PROJECTION_TYPES)
    a = ap.parse_args()
    pt = a.projection_type
    dev = torch.device("cuda:0")
    n, det, V = a.n, a.det, a.views
    angles = np.linspace(0, 2 * np.pi, V + 1)[:-1]
    res = {"case": "%d^3 <- %d x %d^2" % (n, V, det), "reps": a.reps, "run_reps": a.run_reps, "projection_type": pt}
    vol = phantom(n, dev)
    for mode, scanner in (("cone", S.CONE_BEAM), ("parallel", S.PARALLEL_BEAM)):
        views = [S.make_view(float(t), (det, det), scanner) for t in angles]
        p = K.project_views(vol, views, (2.0, 2.0, 2.0), (0.0, 0.0, 0.0), 0.5)
        out = torch.empty_like(vol)
        if pt == "siddon":
            g = (views, (2.0, 2.0, 2.0), (0.0, 0.0, 0.0))
            ms = timed(lambda: RC.backproject_views(p, *g, out=out, projection_type=pt), a.reps, a.warmup)
            fwd = timed(lambda: K.project_views(vol, *g, out=p, projection_type=pt), a.reps, a.warmup)
            ims = timed(lambda: RC.backproject_views(p, *g, 0.5, out=out), a.reps, a.warmup)
            ifwd = timed(lambda: K.project_views(vol, *g, 0.5, out=p), a.reps, a.warmup)
            segments, _ = count_segments(views, n)
            floor = segments * SIDDON_VALU_PER_ENTRY / 64.0 / (CUS * CLOCK) * 1e3
            res["backproject_" + mode] = {"ms": ms, "forward_ms": fwd, "interpolated_ms": ims, "interpolated_forward_ms": ifwd,
                                          "segments": int(segments), "floor_ms_model": floor, "fraction_of_floor": floor / ms}
            continue
        ms = timed(lambda: RC.backproject_views(p, views, (2.0, 2.0, 2.0), (0.0, 0.0, 0.0), 0.5, out=out), a.reps, a.warmup)
        fwd = timed(lambda: K.project_views(vol, views, (2.0, 2.0, 2.0), (0.0, 0.0, 0.0), 0.5, out=p), a.reps, a.warmup)
        samples, _ = count_samples(views, n, 0.5)
        floor = samples * 8 * VALU_PER_VOXEL_SAMPLE / 64.0 / (CUS * CLOCK) * 1e3
        res["backproject_" + mode] = {"ms": ms, "forward_ms": fwd, "samples": int(samples), "floor_ms_model": floor,
                                      "fraction_of_floor": floor / ms}
    x = vol.clone()
    scratch = torch.empty(int(RC._lib.lib().r2_tv_descent_scratch_bytes(n, n, n)), dtype=torch.uint8, device=dev)
    step = torch.full((), 1e-3, device=dev)
    res["tv_step_ms"] = timed(lambda: RC.tv_descent(x, step, 1, scratch), a.reps, a.warmup)
    cfg = dict(S.CONE_BEAM, nVoxel=[n, n, n], nDetector=[det, det], accuracy=0.5, filter=None)
    b = K.project(vol, angles, cfg, projection_type=pt)
    c1 = timed(lambda: RC.cgls(b, angles, cfg, 1, projection_type=pt), a.reps, a.warmup)
    c2 = timed(lambda: RC.cgls(b, angles, cfg, 2, projection_type=pt), a.reps, a.warmup)
    res["cgls_iter_ms"] = c2 - c1
    if a.run_reps > 0:
        res["cgls60_ms"] = timed(lambda: RC.cgls(b, angles, cfg, 60, projection_type=pt), a.run_reps, 0)
        res["sart20_ms"] = timed(lambda: RC.sart(b, angles, cfg, 20, projection_type=pt), a.run_reps, 0)
        res["asd_pocs10_ms"] = timed(lambda: RC.asd_pocs(b, angles, cfg, 10, projection_type=pt), a.run_reps, 0)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
