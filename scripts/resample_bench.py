"""Timing of the cubic-spline resampling kernels (csrc/spline.hip) on the MI355X; prints one JSON line.

    python scripts/resample_bench.py [--rounds 7] [--reps 5] [--no-scipy]

For 256^3 -> 128^3, 512^3 -> 256^3 and 300 x 300 x 200 -> 256^3 on uniform random data (seeded), each pass of the prefilter
(r2_spline_prefilter_pass, axes 0, 1, 2) and the zoom (r2_spline_zoom: its table launch and the 64-tap kernel) are called
through the C ABI, --reps calls between two device events, after one warm-up call each; the median and the minimum over
--rounds windows are reported per call.  The rounds alternate between the four entries, so a clock or a neighbour's load
that drifts during the run meets all of them alike.  Other people's work shares the machine: compare numbers of one run only.

Bytes.  floor_bytes is what an entry must move when every array is read or written once: the x pass reads the volume and
writes the padded block, the y and z passes read and write the padded block, the zoom reads the padded block and writes the
output.  kernel_bytes is what the kernels as written move: a pass writes its causal sweep and reads it back for the
anti-causal one, two more trips of the padded block.  floor_ms = floor_bytes over COPY_BW, the measured float4 copy rate of
the chip, not the 8 TB/s of the data sheet.

Where scipy imports, scipy.ndimage.zoom(mode="nearest") on the same float32 data is timed on the host (one call), next to
the sum of the four device entries.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from r2_gaussian_amd import _lib              # noqa: E402

COPY_BW = 6.29e12   # bytes / s: the chip's measured float4 copy rate
PAD = _lib.R2_SPLINE_PAD
CASES = [((256, 256, 256), (128, 128, 128)), ((512, 512, 512), (256, 256, 256)), ((300, 300, 200), (256, 256, 256))]


def event_ms(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def time_case(shape, out_shape, rounds, reps, dev, with_scipy):
    L = _lib.lib()
    g = torch.Generator(device=dev).manual_seed(sum(shape))
    vol = torch.rand(shape, device=dev, generator=g)
    padded = tuple(n + 2 * PAD for n in shape)
    coeffs = torch.empty(padded, device=dev)
    out = torch.empty(out_shape, device=dev)
    ws = torch.empty(int(L.r2_spline_zoom_workspace_bytes(*out_shape)), dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream

    def check(rc, what):
        if rc != 0:
            raise RuntimeError("%s failed: %d" % (what, rc))

    def run_pass(axis):
        check(L.r2_spline_prefilter_pass(*shape, vol.data_ptr(), coeffs.data_ptr(), axis, stream), "r2_spline_prefilter_pass")

    def run_zoom():
        check(L.r2_spline_zoom(*shape, coeffs.data_ptr(), *out_shape, out.data_ptr(), ws.data_ptr(), ws.numel(), stream),
              "r2_spline_zoom")

    N, P, M = int(np.prod(shape)), int(np.prod(padded)), int(np.prod(out_shape))
    entries = {"pass_x": (lambda: run_pass(0), (N + P) * 4, (N + 3 * P) * 4), "pass_y": (lambda: run_pass(1), 2 * P * 4, 4 * P * 4),
               "pass_z": (lambda: run_pass(2), 2 * P * 4, 4 * P * 4), "zoom": (run_zoom, (P + M) * 4, (P + M) * 4)}
    for fn, _, _ in entries.values():   # warm-up, and the coefficients of the volume for the zoom
        fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in entries}
    for _ in range(rounds):
        for k, (fn, _, _) in entries.items():
            ts[k].append(event_ms(fn, reps))
    res = {"case": "%s -> %s" % ("x".join(map(str, shape)), "x".join(map(str, out_shape)))}
    for k, (_, floor_bytes, kernel_bytes) in entries.items():
        ms = float(np.median(ts[k]))
        res[k] = {"ms": ms, "ms_min": float(np.min(ts[k])), "floor_bytes": floor_bytes, "kernel_bytes": kernel_bytes,
                  "floor_ms": floor_bytes / COPY_BW * 1e3, "gbps": kernel_bytes / (ms * 1e-3) / 1e9}
    res["total_ms"] = float(sum(res[k]["ms"] for k in entries))
    res["z_over_x"] = res["pass_z"]["ms"] / res["pass_x"]["ms"]
    if with_scipy:
        try:
            import scipy.ndimage as ndimage
        except ImportError:
            ndimage = None
        if ndimage is not None:
            host = vol.cpu().numpy()
            t0 = time.perf_counter()
            ndimage.zoom(host, tuple(m / n for m, n in zip(out_shape, shape)), mode="nearest")
            res["scipy_host_ms"] = (time.perf_counter() - t0) * 1e3
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-scipy", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("resample_bench needs the GPU: a timing taken anywhere else says nothing")
    dev = torch.device("cuda:0")
    res = {"rounds": a.rounds, "reps": a.reps, "cases": [time_case(s, o, a.rounds, a.reps, dev, not a.no_scipy) for s, o in CASES]}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
