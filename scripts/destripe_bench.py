"""Timing of the stripe-removal kernels (csrc/destripe.hip) on the MI355X; prints one JSON line.

    python scripts/destripe_bench.py [--rounds 5] [--reps 3] [--torch_rounds 3]

Two stacks of uniform random projections (seeded): 721 views of 560 x 560 (a FIPS scan after the converter's resize; 904 MB, well
beyond the 256 MiB Infinity Cache) and 360 views of 256 x 256 (94 MB, inside it).  On each, through the C ABI:
r2_proj_destripe_sort and r2_proj_destripe_mean (with the offsets) at k = 9 and k = 31.  --reps calls between two device
events, after one warm-up call each; the median and the minimum over --rounds windows are reported per call.  The rounds
alternate between the entries, so a clock or a neighbour's load that drifts during the run meets all of them alike.  Other
people's work shares the machine: compare numbers of one run only.

floor_bytes is the stack read once and written once; floor_ms = floor_bytes over HBM_PEAK, the 8 TB/s of the data sheet that
bench.py measures against (the chip's measured copy rate is 6.29 TB/s); frac = floor_ms / ms.

torch_sort is the same operator composed of library calls, timed in the same run: ``torch.sort(stable=True)`` along dim 0, the
median over an ``unfold`` of the replicate-padded sorted tensor, ``scatter_`` -- one call between two events per round, the
median over --torch_rounds.  ratio = torch ms / r2_proj_destripe_sort ms: the hand-written path has no reason to exist below 1.
On the smaller stack the two results are also compared (equal_to_torch).
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
CASES = [(721, 560, 560), (360, 256, 256)]
SIZES = (9, 31)


def event_ms(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def torch_sort_destripe(src, k):
    S, I = torch.sort(src, dim=0, stable=True)
    padded = torch.nn.functional.pad(S, (k // 2, k // 2), mode="replicate")
    M = padded.unfold(2, k, 1).median(dim=-1).values
    return torch.empty_like(src).scatter_(0, I, M)


def time_case(V, H, W, rounds, reps, torch_rounds, dev):
    L = _lib.lib()
    g = torch.Generator(device=dev).manual_seed(V + H + W)
    src = torch.rand((V, H, W), device=dev, generator=g)
    dst = torch.empty_like(src)
    offsets = torch.empty((H, W), device=dev)
    ws = torch.empty(max(int(L.r2_proj_destripe_workspace_bytes(V, H, W, m)) for m in (0, 1)), dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream

    def check(rc, what):
        if rc != 0:
            raise RuntimeError("%s failed: %d" % (what, rc))

    def sort(k):
        check(L.r2_proj_destripe_sort(V, H, W, src.data_ptr(), k, dst.data_ptr(), ws.data_ptr(), ws.numel(), stream), "r2_proj_destripe_sort")

    def mean(k):
        check(L.r2_proj_destripe_mean(V, H, W, src.data_ptr(), k, dst.data_ptr(), offsets.data_ptr(), ws.data_ptr(), ws.numel(), stream),
              "r2_proj_destripe_mean")

    entries = {}
    for k in SIZES:
        entries["sort%d" % k] = lambda k=k: sort(k)
        entries["mean%d" % k] = lambda k=k: mean(k)
    for fn in entries.values():
        fn()
    torch.cuda.synchronize()
    ts = {name: [] for name in entries}
    for _ in range(rounds):
        for name, fn in entries.items():
            ts[name].append(event_ms(fn, reps))
    floor_bytes = 2 * V * H * W * 4
    res = {"case": "%d x %d x %d" % (V, H, W), "input_MB": V * H * W * 4 / 1e6, "floor_bytes": floor_bytes,
           "floor_ms": floor_bytes / HBM_PEAK * 1e3, "floor_ms_copy_rate": floor_bytes / COPY_BW * 1e3}
    for name in entries:
        ms = float(np.median(ts[name]))
        res[name] = {"ms": ms, "ms_min": float(np.min(ts[name])), "frac": floor_bytes / HBM_PEAK * 1e3 / ms}
    for k in SIZES:
        out = torch_sort_destripe(src, k)   # warm-up: the allocator then holds the composition's temporaries
        if V * H * W <= 2 ** 25:
            sort(k)
            res["sort%d" % k]["equal_to_torch"] = bool(torch.equal(out, dst))
        del out
        torch.cuda.synchronize()
        tt = [event_ms(lambda: torch_sort_destripe(src, k), 1) for _ in range(torch_rounds)]
        ms = float(np.median(tt))
        res["torch_sort%d" % k] = {"ms": ms, "ms_min": float(np.min(tt)), "ratio": ms / res["sort%d" % k]["ms"]}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--torch_rounds", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("destripe_bench needs the GPU: a timing taken anywhere else says nothing")
    dev = torch.device("cuda:0")
    res = {"rounds": a.rounds, "reps": a.reps, "torch_rounds": a.torch_rounds,
           "cases": [time_case(*c, a.rounds, a.reps, a.torch_rounds, dev) for c in CASES]}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
