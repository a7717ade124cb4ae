"""Timing of the volume forward projector (csrc/projector.hip) on the MI355X; prints one JSON line.

    python scripts/project_bench.py [--reps 7] [--warmup 2] [--projection_type interpolated|siddon]

Cases: 50 and 100 views of 512^2 from 256^3 at accuracy 0.5, cone and parallel; 50 views of 256^2 from 128^3.  Each is the
median over --reps calls (HIP events around one project_views call) after --warmup calls.  Reported beside the time:

* samples: the trilinear samples the kernel takes, counted on the host from the clipped chords (the restatement's n per
  ray, in float64), and G samples/s;
* floor_ms, a MODEL, not a measurement: the larger of (a) the gather issue bound, 8 dword gathers per sample, one
  64-lane gather wave-instruction per 4 cycles per CU (64 B/clk per CU vector L1), 256 CUs at 2.4 GHz, and (b) the VALU
  bound, VALU_PER_SAMPLE wave64 instructions per sample (counted from the loop's ISA), 4 SIMDs per CU issuing one per cycle
  each over 4 cycles (wave64 on SIMD16);
* grid_sample_ms: the same sampling restated in torch (grid_sample, trilinear, zero padding, one view at a time, the
  per-ray sample positions precomputed outside the timed region), for the 256^2 / 128^3 case only: its sample tensor for
  a 512^2 view at 256^3 alone is several GB.

With --projection_type siddon the cases are timed with the Siddon projector (csrc/projector_siddon.hip) and, in the same run,
with the interpolated one at accuracy 0.5 beside it (interpolated_ms).  segments: the cells the walks visit, counted on the host
from the clipped chords (1 + the plane crossings inside each chord, float64), and G segments/s.  Its floor_ms is again a
MODEL: one dword gather per segment against SIDDON_VALU_PER_SEGMENT wave64 VALU instructions per segment (counted from the
walk's loop in the gfx950 ISA, all three axis branches, since the lanes of a wave diverge over them); the VALU bound is the
larger by far.  The model assumes the gathers overlap the arithmetic.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from r2_gaussian_amd import projector as K   # noqa: E402
from r2_gaussian_amd import scene as S       # noqa: E402

CUS, CLOCK = 256, 2.4e9
GATHER_CYCLES = 4.0
VALU_PER_SAMPLE = 95.0   # VALU instructions in the sampling loop of project_kernel<unsigned> (gfx950 ISA)
SIDDON_VALU_PER_SEGMENT = 34.0   # VALU instructions per iteration of project_siddon_kernel<unsigned>'s walk (gfx950 ISA)


def count_segments(views, n):
    """sum over hit rays of 1 + the number of voxel planes crossed inside the chord clipped to [-1/2, n - 1/2]^3 (float64)."""
    rays = K.ray_params(views, (2.0, 2.0, 2.0), (0.0, 0.0, 0.0), (n, n, n)).astype(np.float64)
    H, W = views[0].image_height, views[0].image_width
    rr, cc = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    total, hits = 0, 0
    for v, R in zip(views, rays):
        P = R[3:6] + cc[..., None] * R[6:9] + rr[..., None] * R[9:12]
        if v.mode == 1:
            Sx, Dx = np.broadcast_to(R[0:3], P.shape), P - R[0:3]
        else:
            Sx, Dx = P, np.broadcast_to(R[0:3], P.shape)
        with np.errstate(divide="ignore", invalid="ignore"):
            ta, tb = (-0.5 - Sx) / Dx, (n - 0.5 - Sx) / Dx
            lo = np.where(Dx != 0, np.minimum(ta, tb), -np.inf).max(-1)
            hi = np.where(Dx != 0, np.maximum(ta, tb), np.inf).min(-1)
        if v.mode == 1:
            lo = np.maximum(lo, 0.0)
        hit = hi > lo
        lo, hi = np.where(hit, lo, 0.0), np.where(hit, hi, 0.0)
        # the cells of the chord's two ends: the planes crossed between them, axis by axis
        ca = np.clip(np.floor(Sx + lo[..., None] * Dx + 0.5), 0, n - 1)
        cb = np.clip(np.floor(Sx + hi[..., None] * Dx + 0.5), 0, n - 1)
        total += int(np.where(hit, 1 + np.abs(cb - ca).sum(-1), 0).sum())
        hits += int(hit.sum())
    return total, hits


def count_samples(views, n, accuracy):
    """sum over rays of max(1, ceil(L / accuracy)) for hit rays (float64 clip of the product's float32 ray parameters)."""
    rays = K.ray_params(views, (2.0, 2.0, 2.0), (0.0, 0.0, 0.0), (n, n, n)).astype(np.float64)
    H, W = views[0].image_height, views[0].image_width
    rr, cc = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    total, hits = 0, 0
    for v, R in zip(views, rays):
        P = R[3:6] + cc[..., None] * R[6:9] + rr[..., None] * R[9:12]
        if v.mode == 1:
            Sx, Dx = np.broadcast_to(R[0:3], P.shape), P - R[0:3]
        else:
            Sx, Dx = P, np.broadcast_to(R[0:3], P.shape)
        with np.errstate(divide="ignore", invalid="ignore"):
            ta, tb = (-1.0 - Sx) / Dx, (n - Sx) / Dx
            lo = np.where(Dx != 0, np.minimum(ta, tb), -np.inf).max(-1)
            hi = np.where(Dx != 0, np.maximum(ta, tb), np.inf).min(-1)
        if v.mode == 1:
            lo = np.maximum(lo, 0.0)
        hit = hi > lo
        L = np.where(hit, hi - lo, 0.0) * np.linalg.norm(Dx, axis=-1)
        total += int(np.where(hit, np.maximum(1, np.ceil(L / accuracy)), 0).sum())
        hits += int(hit.sum())
    return total, hits


def time_call(fn, reps, warmup):
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
    return float(np.median(ts)), float(min(ts)), float(max(ts))


def grid_sample_restatement(vol, views, accuracy, dev):
    """-> a closure computing the same projections with torch grid_sample, one view at a time (sample positions and
    weights prepared on the device in float64 beforehand, outside the timed closure)."""
    n = vol.shape[0]
    rays = torch.from_numpy(K.ray_params(views, (2.0, 2.0, 2.0), (0.0, 0.0, 0.0), (n, n, n))).to(dev, torch.float64)
    H, W = views[0].image_height, views[0].image_width
    rr, cc = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float64),
                            torch.arange(W, device=dev, dtype=torch.float64), indexing="ij")
    rr, cc = rr.reshape(-1, 1), cc.reshape(-1, 1)
    per_view = []
    for v, R in zip(views, rays):
        P = R[3:6] + cc * R[6:9] + rr * R[9:12]
        Sx, Dx = (R[0:3].expand_as(P), P - R[0:3]) if v.mode == 1 else (P, R[0:3].expand_as(P))
        ta, tb = (-1.0 - Sx) / Dx, (n - Sx) / Dx
        lo = torch.where(Dx != 0, torch.minimum(ta, tb), -torch.inf).amax(-1)
        hi = torch.where(Dx != 0, torch.maximum(ta, tb), torch.inf).amin(-1)
        if v.mode == 1:
            lo = lo.clamp_min(0.0)
        hit = hi > lo
        span = torch.where(hit, hi - lo, 0.0)
        ns = torch.where(hit, torch.ceil(span * Dx.norm(dim=-1) / accuracy).clamp_min(1), 0).long()
        ray = torch.repeat_interleave(torch.arange(len(P), device=dev), ns)
        k = torch.arange(len(ray), device=dev, dtype=torch.float64) - torch.repeat_interleave(torch.cumsum(ns, 0) - ns, ns) + 0.5
        dt = span / ns.clamp_min(1)
        q = Sx[ray] + (lo[ray] + k * dt[ray])[:, None] * Dx[ray]
        # grid_sample (align_corners=True): x <-> last axis (nz), index i <-> -1 + 2 i / (n - 1)
        g = (2.0 * q.flip(-1) / (n - 1) - 1.0).float().view(1, 1, 1, -1, 3)
        w = (dt * (Dx * (2.0 / n)).norm(dim=-1)).float()
        per_view.append((g, ray, w))
    v5 = vol.view(1, 1, n, n, n)

    def run():
        out = torch.zeros(len(views), H * W, device=dev)
        for i, (g, ray, w) in enumerate(per_view):
            s = torch.nn.functional.grid_sample(v5, g, mode="bilinear", padding_mode="zeros", align_corners=True).view(-1)
            out[i].index_add_(0, ray, s)
            out[i].mul_(w)
        return out.view(len(views), H, W)
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--projection_type", default="interpolated", choices=K.PROJECTION_TYPES)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator(device="cpu").manual_seed(0)
    result = {"device": torch.cuda.get_device_name(0), "cases": []}
    for (n, det, V, mode) in ((256, 512, 50, "cone"), (256, 512, 50, "parallel"), (256, 512, 100, "cone"),
                              (256, 512, 100, "parallel"), (128, 256, 50, "cone")):
        vol = torch.rand(n, n, n, generator=g).to(dev)
        scanner = S.CONE_BEAM if mode == "cone" else S.PARALLEL_BEAM
        views = [S.make_view(a, (det, det), scanner) for a in np.linspace(0, 2 * np.pi, V + 1)[:-1]]
        out = torch.empty(V, det, det, device=dev)
        if args.projection_type == "siddon":
            sargs = (vol, views, (2.0, 2.0, 2.0), (0.0, 0.0, 0.0))
            med, lo, hi = time_call(lambda: K.project_views(*sargs, out=out, projection_type="siddon"), args.reps, args.warmup)
            imed, _, _ = time_call(lambda: K.project_views(*sargs, 0.5, out=out), args.reps, args.warmup)
            segments, hits = count_segments(views, n)
            floor_valu = segments / 64.0 * SIDDON_VALU_PER_SEGMENT * 4.0 / (4 * CUS * CLOCK) * 1e3
            floor_gather = segments / 64.0 * GATHER_CYCLES / (CUS * CLOCK) * 1e3
            result["cases"].append({"vol": n, "det": det, "views": V, "mode": mode, "projection_type": "siddon",
                                    "ms_median": med, "ms_min": lo, "ms_max": hi, "interpolated_ms": imed,
                                    "segments": segments, "hit_rays_fraction": hits / float(V * det * det),
                                    "gsegments_per_s": segments / (med * 1e-3) / 1e9,
                                    "floor_ms_model": max(floor_valu, floor_gather), "floor_gather_ms_model": floor_gather,
                                    "floor_valu_ms_model": floor_valu, "fraction_of_floor": max(floor_valu, floor_gather) / med})
            del vol, out
            torch.cuda.empty_cache()
            continue
        med, lo, hi = time_call(lambda: K.project_views(vol, views, (2.0, 2.0, 2.0), (0.0, 0.0, 0.0), 0.5, out=out),
                                args.reps, args.warmup)
        samples, hits = count_samples(views, n, 0.5)
        waves = samples / 64.0   # wave64 iterations of the sampling loop
        floor_gather = waves * 8 * GATHER_CYCLES / (CUS * CLOCK) * 1e3
        floor_valu = waves * VALU_PER_SAMPLE * 4.0 / (4 * CUS * CLOCK) * 1e3
        floor_ms = max(floor_gather, floor_valu)
        case = {"vol": n, "det": det, "views": V, "mode": mode, "ms_median": med, "ms_min": lo, "ms_max": hi,
                "samples": samples, "hit_rays_fraction": hits / float(V * det * det),
                "gsamples_per_s": samples / (med * 1e-3) / 1e9, "floor_ms_model": floor_ms,
                "floor_gather_ms_model": floor_gather, "floor_valu_ms_model": floor_valu,
                "fraction_of_floor": floor_ms / med}
        if n == 128:
            run = grid_sample_restatement(vol, views, 0.5, dev)
            ref = run()
            case["grid_sample_max_rel_diff"] = float((ref - out).abs().max() / out.abs().max())
            gmed, _, _ = time_call(run, max(3, args.reps // 2), 1)
            case["grid_sample_ms"] = gmed
            case["speedup_vs_grid_sample"] = gmed / med
        result["cases"].append(case)
        del vol, out
        torch.cuda.empty_cache()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
