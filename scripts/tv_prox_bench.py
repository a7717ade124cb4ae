"""Timing of the TV proximal operator (csrc/tv_prox.hip) and of FISTA-TV (recon.fista_tv) on the MI355X, and the sweep that
chose fista_tv's defaults; prints one JSON line.

    python scripts/tv_prox_bench.py [--rounds 9] [--iters 100] [--alt-lib r2_gaussian_amd/libr2hip_tvprox2.so]
    python scripts/tv_prox_bench.py --sweep

Timing.  For 128^3 and 256^3 volumes of uniform random data (seeded), r2_tv_prox is called through the C ABI with 1 and with
1 + --iters iterations; per_iter_ms is the difference of the two medians over --iters, so the output pass and the launch of
the call drop out.  Every timed window is a whole call of --iters iterations between two device events (tens of
milliseconds at 256^3), after one warm-up call per library and size.  The rounds ALTERNATE between the libraries and between
the two iteration counts, so a clock or a neighbour's load that drifts during the run meets all of them alike; the medians
and the minima over the rounds are both reported.  Other people's work shares the machine and its clocks: compare numbers
of one run only.

--alt-lib names a second build of the library to time beside the product one in the same process: the two-launch iteration
is such a build,

    python -m r2_gaussian_amd.build -DR2_TV_PROX_TWO_LAUNCH=1 --out=libr2hip_tvprox2.so

and the run also checks that both libraries return the same bits.

Bytes.  bytes_per_iter is what one iteration must move when every array is read or written once and neighbours come from
cache: the one-launch iteration reads y, r (3) and p (3) and writes r (3) and p (3), 13 floats per voxel (its halo re-reads
are overhead above that); the two-launch iteration moves 18 (x_k goes to memory and comes back).  gbps = the library's own
bytes_per_iter over per_iter_ms; floor_ms = bytes_per_iter over COPY_BW, the measured float4 copy rate of the chip, not the
8 TB/s of the data sheet.

FISTA.  At 256^3 <- 50 x 512^2 (cone beam, accuracy 0.5) one iteration of fista_tv (A, A^T, the vector updates and tviter
TV iterations) is timed as the difference of the medians of runs with 2 and with 1 iterations, next to one CGLS iteration and
one SART sweep measured the same way.

--sweep.  The anchor of tests/test_tv_prox_gpu.py: 64^3 phantom, 20 cone views of 96^2 with datagen.noisy_train noise (seed 0);
fista_tv with 50 iterations over a decade grid of lam (relative to |A^T b|_inf) and three values of tviter; 3-D PSNR
against the phantom and the TV of the result, next to SART-10 on the same data.
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
from r2_gaussian_amd import datagen as D      # noqa: E402
from r2_gaussian_amd import projector as K    # noqa: E402
from r2_gaussian_amd import recon as RC       # noqa: E402
from r2_gaussian_amd import scene as S        # noqa: E402

COPY_BW = 6.29e12   # bytes / s: the chip's measured float4 copy rate
FLOATS_PER_ITER = {"one_launch": 13, "two_launch": 18}


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def time_prox(libs, n, iters, rounds, dev):
    g = torch.Generator(device=dev).manual_seed(n)
    y = torch.rand((n, n, n), device=dev, generator=g)
    lam = torch.full((), 0.1, device=dev)
    scratch = torch.empty(int(_lib.lib().r2_tv_prox_scratch_bytes(n, n, n)), dtype=torch.uint8, device=dev)
    outs = {k: torch.empty_like(y) for k in libs}
    stream = torch.cuda.current_stream(dev).cuda_stream

    def run(name, k):
        rc = libs[name].r2_tv_prox(n, n, n, y.data_ptr(), outs[name].data_ptr(), lam.data_ptr(), k, 0.0, float("inf"),
                                   scratch.data_ptr(), scratch.numel(), stream)
        if rc != 0:
            raise RuntimeError("r2_tv_prox failed in %s: %d" % (name, rc))

    for name in libs:   # warm-up: both kernels of every library at this size
        run(name, 3)
    torch.cuda.synchronize()
    ts = {(name, k): [] for name in libs for k in (1, 1 + iters)}
    for _ in range(rounds):
        for k in (1, 1 + iters):
            for name in libs:
                ts[(name, k)].append(event_ms(lambda: run(name, k)))
    res = {}
    for name in libs:
        per = (np.median(ts[(name, 1 + iters)]) - np.median(ts[(name, 1)])) / iters
        per_min = (np.min(ts[(name, 1 + iters)]) - np.min(ts[(name, 1)])) / iters
        nbytes = FLOATS_PER_ITER[name] * 4 * n ** 3
        res[name] = {"per_iter_ms": float(per), "per_iter_ms_min": float(per_min), "bytes_per_iter": nbytes,
                     "gbps": nbytes / (per * 1e-3) / 1e9, "floor_ms": nbytes / COPY_BW * 1e3,
                     "fraction_of_floor": nbytes / COPY_BW * 1e3 / float(per), "call_1_iter_ms": float(np.median(ts[(name, 1)]))}
    names = list(libs)
    if len(names) > 1:
        res["same_bits"] = all(bool(torch.equal(outs[names[0]], outs[k])) for k in names[1:])
    return res


def median_of(fn, reps):
    fn()
    torch.cuda.synchronize()
    return float(np.median([event_ms(fn) for _ in range(reps)]))


def time_fista(n, det, V, reps, dev):
    angles = np.linspace(0, 2 * np.pi, V + 1)[:-1]
    cfg = dict(S.CONE_BEAM, nVoxel=[n, n, n], nDetector=[det, det], accuracy=0.5, filter=None)
    ax = torch.linspace(-1 + 1.0 / n, 1 - 1.0 / n, n, device=dev)
    X, Y, Z = torch.meshgrid(ax, ax, ax, indexing="ij")
    vol = (0.6 * torch.exp(-((X - 0.1) ** 2 + (Y + 0.2) ** 2 + Z ** 2) / 0.18)).contiguous()
    b = K.project(vol, angles, cfg)
    res = {"case": "%d^3 <- %d x %d^2" % (n, V, det), "tviter": RC.FISTA_TVITER}
    for name, fn in (("fista_tv", lambda k: RC.fista_tv(b, angles, cfg, k)), ("cgls", lambda k: RC.cgls(b, angles, cfg, k)),
                     ("sart", lambda k: RC.sart(b, angles, cfg, k))):
        # alternate the two iteration counts
        t1, t2 = [], []
        fn(1)
        torch.cuda.synchronize()
        for _ in range(reps):
            t1.append(event_ms(lambda: fn(1)))
            t2.append(event_ms(lambda: fn(2)))
        res[name + "_iter_ms"] = float(np.median(t2) - np.median(t1))
    return res


def _blob(n, c0, sigma, rho):
    ax = -1 + (np.arange(n) + 0.5) * 2.0 / n
    X, Y, Z = np.meshgrid(ax, ax, ax, indexing="ij")
    return (rho * np.exp(-((X - c0[0]) ** 2 + (Y - c0[1]) ** 2 + (Z - c0[2]) ** 2) / (2 * sigma ** 2))).astype(np.float32)


def sweep(dev):
    from r2_gaussian_amd.metrics import metric_vol
    n = 64
    vol = _blob(n, (0.1, -0.2, 0.05), 0.3, 0.6) + _blob(n, (-0.3, 0.25, -0.1), 0.12, 0.5) + _blob(n, (0.35, 0.3, 0.2), 0.08, 0.4)
    cfg = dict(S.CONE_BEAM, nVoxel=[n, n, n], nDetector=[96, 96], accuracy=0.5, filter=None, noise=True, possion_noise=10000,
               gaussian_noise=[0, 10])
    angles = np.linspace(0, 2 * np.pi, 21)[:-1]
    noisy = D.noisy_train(K.project(vol, angles, cfg).cpu().numpy(), cfg, np.random.RandomState(0))
    xs = RC.sart(noisy, angles, cfg, 10)
    res = {"case": "64^3 <- 20 x 96^2, noisy", "niter": 50,
           "sart10": {"psnr": float(metric_vol(vol, xs.cpu().numpy(), "psnr")[0]), "tv": float(RC.tv_value(xs))}, "rows": []}
    for tviter in (10, 20, 50):
        for lam in (1e-5, 1e-4, 1e-3, 1e-2, 1e-1):
            x = RC.fista_tv(noisy, angles, cfg, 50, lam, tviter)
            res["rows"].append({"lam": lam, "tviter": tviter, "psnr": float(metric_vol(vol, x.cpu().numpy(), "psnr")[0]),
                                "tv": float(RC.tv_value(x))})
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--sizes", type=int, nargs="+", default=[128, 256])
    ap.add_argument("--alt-lib", default=None, help="a second build of the library (the two-launch iteration)")
    ap.add_argument("--fista-reps", type=int, default=5)
    ap.add_argument("--sweep", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tv_prox_bench needs the GPU: a timing taken anywhere else says nothing")
    dev = torch.device("cuda:0")
    if a.sweep:
        print(json.dumps(sweep(dev)))
        return
    libs = {"one_launch": _lib.bind(_lib.LIB_PATH)}
    if a.alt_lib:
        libs["two_launch"] = _lib.bind(os.path.abspath(a.alt_lib))
    res = {"rounds": a.rounds, "iters": a.iters}
    for n in a.sizes:
        res["prox_%d" % n] = time_prox(libs, n, a.iters, a.rounds, dev)
    if a.fista_reps > 0:
        res["fista"] = time_fista(256, 512, 50, a.fista_reps, dev)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
