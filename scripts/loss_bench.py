"""The fused image loss at 512^2, one view and V = 4, 8 views per call: the weighted entries against the unweighted ones of
this build, and the unweighted ones of this build against those of another build of the library (the parent commit's
libr2hip.so), alternating on ONE box.

    python scripts/loss_bench.py [--parent path/to/libr2hip.so] [--size 512] [--calls 4000] [--rounds 9] [--out file.json]

A round times every variant once, in an order that rotates from round to round: `calls` back-to-back calls through the C ABI
on preallocated buffers, a host clock around them and a device synchronise at both ends (us per call).  Per variant: the
median over the rounds and the spread (max - min over the rounds) -- the run-to-run noise a difference has to exceed to mean
anything.  Before timing, the unweighted outputs of the two libraries are compared bit for bit, and the weighted call with
unit weights against the unweighted one.  Weighted variants: `mask` (30 % zeros, NaN measurements under them) and `null`
(weights == NULL: the weighted kernels on unit weights).  Prints one line per variant and one JSON line; nothing is asserted
about the weighted cost."""
import argparse
import ctypes as C
import json
import statistics
import sys
import time

import torch

sys.path.insert(0, ".")
from r2_gaussian_amd import _lib
from r2_gaussian_amd._boundary import ptr_table

NAMES = ("r2_loss_l1_ssim_scratch_floats", "r2_loss_l1_ssim", "r2_loss_l1_ssim_batch_scratch_floats", "r2_loss_l1_ssim_batch")


def load_other(path):
    """Another build of the library with the unweighted entries' ctypes signatures of this one."""
    L = C.CDLL(path)
    for n in NAMES:
        fn = getattr(L, n)
        fn.restype, fn.argtypes = _lib._SIGNATURES[n]
    return L


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--parent", default=None, help="libr2hip.so of the build to compare the unweighted loss against")
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--calls", type=int, default=4000)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        sys.exit("loss_bench needs a GPU: a timing taken anywhere else says nothing")
    dev = torch.device("cuda:0")
    here = _lib.lib()
    libs = {"this": here}
    if args.parent:
        libs["parent"] = load_other(args.parent)
    n, lam = args.size, 0.25
    gen = torch.Generator().manual_seed(0)
    result = {"size": n, "calls": args.calls, "rounds": args.rounds, "variants": {}}
    for V in (1, 4, 8):
        gt = torch.rand((V, n, n), generator=gen)
        img = (gt + 0.1 * torch.randn((V, n, n), generator=gen)).clamp_(min=0).to(dev)
        w = (2.0 * torch.rand((V, n, n), generator=gen) * (torch.rand((V, n, n), generator=gen) > 0.3)).to(dev)
        gt_nan = torch.where(w.cpu() > 0, gt, torch.full_like(gt, float("nan"))).to(dev)
        gt = gt.to(dev)
        ones = torch.ones_like(w)
        grad = torch.empty_like(img)
        if V == 1:
            ns, nw = here.r2_loss_l1_ssim_scratch_floats(n, n), here.r2_loss_l1_ssim_weighted_scratch_floats(n, n)
        else:
            ns, nw = (here.r2_loss_l1_ssim_batch_scratch_floats(V, n, n), here.r2_loss_l1_ssim_weighted_batch_scratch_floats(V, n, n))
        scratch = torch.empty(max(ns, nw), device=dev)
        scalars = torch.empty((V + 1) * 4, device=dev)
        p = lambda t: t.data_ptr()
        tab = lambda t: ptr_table(list(t))

        def unweighted(L):
            if V == 1:
                return lambda: L.r2_loss_l1_ssim(n, n, p(img), p(gt), 1.0, lam, p(grad), p(scratch), p(scalars), None)
            t = tab(gt)
            return lambda: L.r2_loss_l1_ssim_batch(V, n, n, p(img), t, 1.0, lam, p(grad), p(scratch), p(scalars), None)

        def weighted(y, wts):
            if V == 1:
                return lambda: here.r2_loss_l1_ssim_weighted(n, n, p(img), p(y), None if wts is None else p(wts), 1.0, lam, p(grad),
                                                             p(scratch), p(scalars), None)
            t, tw = tab(y), None if wts is None else tab(wts)
            return lambda: here.r2_loss_l1_ssim_weighted_batch(V, n, n, p(img), t, tw, 1.0, lam, p(grad), p(scratch), p(scalars), None)

        variants = {"unweighted/" + k: unweighted(L) for k, L in libs.items()}
        variants["weighted/mask"] = weighted(gt_nan, w)
        variants["weighted/null"] = weighted(gt, None)

        def outputs(fn):
            grad.zero_()
            scalars.zero_()
            if fn() != 0:
                sys.exit("a call failed: %s" % here.r2_last_error())
            torch.cuda.synchronize()
            return grad.clone().view(torch.int32), scalars.clone().view(torch.int32).view(V + 1, 4)
        base_g, base_s = outputs(variants["unweighted/this"])
        rows = 1 if V == 1 else V + 1
        base_s = base_s.reshape(-1)[:3 * rows].view(rows, 3)
        same = {}
        if "parent" in libs:
            g, s = outputs(variants["unweighted/parent"])
            same["parent"] = bool(torch.equal(g, base_g) and torch.equal(s.reshape(-1)[:3 * rows].view(rows, 3), base_s))
        for name, fn in (("null", variants["weighted/null"]), ("ones", weighted(gt, ones))):
            g, s = outputs(fn)
            same[name] = bool(torch.equal(g, base_g) and torch.equal(s[:rows, :3], base_s))
        order = list(variants)
        times = {k: [] for k in order}
        for fn in variants.values():            # warm every variant at this shape
            for _ in range(50):
                fn()
        torch.cuda.synchronize()
        for r in range(args.rounds):
            for k in order[r % len(order):] + order[:r % len(order)]:
                fn = variants[k]
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.calls):
                    fn()
                torch.cuda.synchronize()
                times[k].append((time.perf_counter() - t0) / args.calls * 1e6)
        for k in order:
            ts = times[k]
            rec = {"median_us": statistics.median(ts), "min_us": min(ts), "max_us": max(ts), "spread_us": max(ts) - min(ts)}
            result["variants"]["V%d/%s" % (V, k)] = rec
            print("V %d  %-18s %8.2f us/call  (min %.2f, max %.2f, spread %.2f over %d rounds)" % (
                V, k, rec["median_us"], rec["min_us"], rec["max_us"], rec["spread_us"], args.rounds), flush=True)
        result["V%d/bits" % V] = same
        print("V %d  bit for bit against unweighted/this: %s" % (V, same), flush=True)
        if "parent" in libs:
            a, b = result["variants"]["V%d/unweighted/this" % V], result["variants"]["V%d/unweighted/parent" % V]
            diff, noise = abs(a["median_us"] - b["median_us"]), max(a["spread_us"], b["spread_us"])
            result["V%d/unweighted_agree" % V] = bool(diff <= noise)
            print("V %d  unweighted this vs parent: |difference of medians| %.2f us, run-to-run spread %.2f us: %s" % (
                V, diff, noise, "agree" if diff <= noise else "DIFFER"), flush=True)
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    ok = all(v for k, v in result.items() if k.endswith("/bits") for v in v.values())
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
