"""Device time of the evaluation metrics (csrc/metric_ops.hip, r2_gaussian_amd/metrics.py); prints ONE JSON line.

    python scripts/metrics_bench.py [--reps 30] [--skip-host]

* metric_vol SSIM + PSNR (all three axes: the work of metric_vol_both) at 128^3 and 256^3;
* metric_proj PSNR + SSIM on a 50 x 512^2 stack, passed as train.py does: the [512, 512, 50] view of [50, 512, 512] storage;
* device time = HIP events around the kernels of one call (no host readback), median of --reps calls after warm-up; wall time
  of the full Python call (including its one synchronisation) next to it;
* achieved GB/s = the bytes the algorithm must move (each input read once per axis, the transposed copy of axis 2 written
  and read) over the device time;
* VALU fraction as DESIGN.md section 4 prices it: wave-level VALU instructions x 2.8 cycles / (1024 SIMDs x 2.4 GHz) over the
  device time.  The instruction counts are a model read off the gfx950 ISA of the kernels (per wave, the mean of a block's
  four: SSIM tile 469, SSE / maximum pass 35 + 9 per 64-wide row segment, finish 120, transpose 43), not counters;
* once, the wall time of the host evaluation model_io.metric_vol(..., "ssim") at 256^3 on the CPU threads this process has.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from r2_gaussian_amd import _lib, metrics as Mx, model_io   # noqa: E402

SIMDS, CLOCK, CYCLES = 1024, 2.4e9, 2.8
VALU_SSIM, VALU_FINISH, VALU_T = 469, 120, 43


def device_ms(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out)


def wall_ms(fn, reps):
    fn()
    out = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t) * 1e3)
    return statistics.median(out)


def ceil(a, b):
    return -(-a // b)


def model(shape, axes, ssim, normalize):
    """-> (bytes, VALU wave-instructions) of r2_metric_slices over `axes` of a C-contiguous `shape`."""
    n0, n1, n2 = shape
    N = n0 * n1 * n2
    nbytes, valu = 0, 0
    for ax in axes:
        n, W, H = {0: (n0, n2, n1), 1: (n1, n2, n0), 2: (n2, n1, n0)}[ax]
        if ax == 2:
            nbytes += 4 * 4 * N                                    # both inputs read and written once
            valu += 2 * ceil(n0 * n1, 32) * ceil(n2, 32) * 4 * VALU_T
        passes = 1 + int(normalize)
        nbytes += passes * 2 * 4 * N
        nb = ceil(W, 16) * ceil(H, 16)
        sse_blocks = ceil(H, 16) * n
        sse_wave = 35 + 9 * 4 * ceil(W, 64)                        # 4 rows per wave
        valu += (passes - int(ssim)) * sse_blocks * 4 * sse_wave
        if ssim:
            valu += n * nb * 4 * VALU_SSIM
        valu += passes * n * 4 * VALU_FINISH
    return nbytes, valu


def entry(name, ms, nbytes, valu, wall=None):
    floor_ms = valu * CYCLES / (SIMDS * CLOCK) * 1e3
    e = {"name": name, "device_ms": round(ms, 4), "GBps": round(nbytes / (ms * 1e-3) / 1e9, 1), "bytes": nbytes,
         "valu_instructions_model": valu, "valu_floor_ms": round(floor_ms, 4), "valu_fraction": round(floor_ms / ms, 3)}
    if wall is not None:
        e["wall_ms"] = round(wall, 4)
    return e


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--skip-host", action="store_true", help="leave out the one CPU evaluation at 256^3")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "metrics_bench.py measures the GPU kernels: no GPU visible"
    _lib.lib()
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    res = []
    host = None
    for n in (128, 256):
        gt = torch.rand(n, n, n, device=dev, generator=g)
        pred = (gt + 0.05 * torch.randn(n, n, n, device=dev, generator=g)).clamp_min(0.0)
        perm = [0, 1, 2]
        out = torch.empty(3 * n, 4, device=dev)
        ms = device_ms(lambda: Mx._run(gt, pred, perm, [0, 1, 2], _lib.R2_METRIC_SSIM, out), args.reps)
        wall = wall_ms(lambda: Mx.metric_vol_both(gt, pred), args.reps)
        res.append(entry("metric_vol ssim+psnr %d^3" % n, ms, *model((n, n, n), [0, 1, 2], True, False), wall))
        ms = device_ms(lambda: Mx._run(gt, pred, perm, [0], 0, out), args.reps)
        wall = wall_ms(lambda: Mx.metric_vol(gt, pred, "psnr"), args.reps)
        res.append(entry("metric_vol psnr %d^3" % n, ms, *model((n, n, n), [0], False, False), wall))
        if n == 256 and not args.skip_host:
            a, b = gt.cpu(), pred.cpu()
            t = time.perf_counter()
            model_io.metric_vol(a, b, "ssim")
            host = {"name": "model_io.metric_vol ssim 256^3 (host, CPU)", "wall_ms": round((time.perf_counter() - t) * 1e3, 1),
                    "cpu_threads": torch.get_num_threads()}
    N, H, W = 50, 512, 512
    gt = torch.rand(N, H, W, device=dev, generator=g)
    pred = (gt + 0.05 * torch.randn(N, H, W, device=dev, generator=g)).clamp_min(0.0)
    vg, vp = gt.permute(1, 2, 0), pred.permute(1, 2, 0)
    out = torch.empty(N, 4, device=dev)
    perm = Mx._storage_order(vg)
    for m, fl in (("psnr", _lib.R2_METRIC_NORMALIZE), ("ssim", _lib.R2_METRIC_NORMALIZE | _lib.R2_METRIC_SSIM)):
        ms = device_ms(lambda: Mx._run(vg, vp, perm, [2], fl, out), args.reps)
        wall = wall_ms(lambda: Mx.metric_proj(vg, vp, m), args.reps)
        res.append(entry("metric_proj %s 50x512^2" % m, ms, *model((N, H, W), [0], m == "ssim", True), wall))
    line = {"metrics_bench": res, "host": host, "device": torch.cuda.get_device_name(0), "reps": args.reps}
    print(json.dumps(line))


if __name__ == "__main__":
    main()
