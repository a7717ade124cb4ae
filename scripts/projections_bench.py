"""Timing of the projection-conditioning kernels (csrc/projections.hip) on the MI355X; prints one JSON line.

    python scripts/projections_bench.py [--rounds 7] [--reps 20]

Two stacks of uniform random projections (seeded), each larger than the 256 MiB Infinity Cache so that a call's input comes
from HBM: 16 views of 2240 x 2368 (a FIPS detector image; 339 MB) and 256 views of 560 x 560 (321 MB).  On each, through the C
ABI: r2_proj_resize as prepare_real.py calls it (shift 5 rows, clamp at 0, a factor of 4 -- 560 x 592 cropped to 560 x 560, and
140 x 140 -- bilinear and box mean) and r2_proj_median (k = 3 and 5, conditional, without the mask).  --reps calls between two
device events, after one warm-up call each; the median and the minimum over --rounds windows are reported per call.  The rounds
alternate between the entries, so a clock or a neighbour's load that drifts during the run meets all of them alike.  Other
people's work shares the machine: compare numbers of one run only.

floor_bytes is what an entry must move when its input is read once and its output written once; floor_ms = floor_bytes over
HBM_PEAK, the 8 TB/s of the data sheet that bench.py measures against (the chip's measured copy rate is 6.29 TB/s);
frac = floor_ms / ms.  The bilinear resize by 4 taps two of every four rows and columns, so it can stay below its floor's
bytes: touched_bytes counts the rows it reads.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from r2_gaussian_amd import _lib              # noqa: E402

HBM_PEAK = 8.0e12    # bytes / s: bench.py's HBM_PEAK_GBS
COPY_BW = 6.29e12    # bytes / s: the chip's measured float4 copy rate
CASES = [(16, 2240, 2368, 560, 592, (0, 16, 560, 560)), (256, 560, 560, 140, 140, (0, 0, 140, 140))]


def event_ms(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def time_case(V, H, W, mh, mw, crop, rounds, reps, dev):
    L = _lib.lib()
    g = torch.Generator(device=dev).manual_seed(V + H + W)
    src = torch.rand((V, H, W), device=dev, generator=g) - 0.2
    r0, c0, oh, ow = crop
    small = torch.empty((V, oh, ow), device=dev)
    full = torch.empty((V, H, W), device=dev)
    ws = torch.empty(int(L.r2_proj_resize_workspace_bytes(mh, mw)), dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream

    def check(rc, what):
        if rc != 0:
            raise RuntimeError("%s failed: %d" % (what, rc))

    def resize(interp):
        check(L.r2_proj_resize(V, H, W, src.data_ptr(), 5, 0, 0.0, interp, mh, mw, r0, c0, oh, ow, small.data_ptr(), ws.data_ptr(),
                               ws.numel(), stream), "r2_proj_resize")

    def median(k):
        check(L.r2_proj_median(V, H, W, src.data_ptr(), k, 1, 0.5, full.data_ptr(), None, stream), "r2_proj_median")

    n_in, n_out = V * H * W * 4, V * oh * ow * 4
    entries = {"resize_linear": (lambda: resize(0), n_in + n_out, n_in // 2 + n_out), "resize_area": (lambda: resize(1), n_in + n_out, n_in + n_out),
               "median3": (lambda: median(3), 2 * n_in, 2 * n_in), "median5": (lambda: median(5), 2 * n_in, 2 * n_in)}
    for fn, _, _ in entries.values():
        fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in entries}
    for _ in range(rounds):
        for k, (fn, _, _) in entries.items():
            ts[k].append(event_ms(fn, reps))
    res = {"case": "%d x %d x %d -> %d x %d, window %s" % (V, H, W, mh, mw, "x".join(map(str, crop[2:]))), "input_MB": n_in / 1e6}
    for k, (_, floor_bytes, touched_bytes) in entries.items():
        ms = float(np.median(ts[k]))
        res[k] = {"ms": ms, "ms_min": float(np.min(ts[k])), "floor_bytes": floor_bytes, "touched_bytes": touched_bytes,
                  "floor_ms": floor_bytes / HBM_PEAK * 1e3, "floor_ms_copy_rate": floor_bytes / COPY_BW * 1e3,
                  "frac": floor_bytes / HBM_PEAK * 1e3 / ms, "gbps": touched_bytes / (ms * 1e-3) / 1e9}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("projections_bench needs the GPU: a timing taken anywhere else says nothing")
    dev = torch.device("cuda:0")
    res = {"rounds": a.rounds, "reps": a.reps, "cases": [time_case(*c, a.rounds, a.reps, dev) for c in CASES]}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
