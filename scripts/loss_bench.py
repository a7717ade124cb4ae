"""The fused image loss at 512^2, one view and V = 4, 8 views per call, and the per-slice SSIM metric of a volume: the weighted
entries against the unweighted ones of this build, and every entry of this build against that of another build of the library
(the parent commit's libr2hip.so), alternating on ONE box.

    python scripts/loss_bench.py [--parent path/to/libr2hip.so] [--size 512] [--volume 96 128 160] [--calls 4000] [--rounds 9]
                                 [--out file.json]

A round times every variant once, in an order that rotates from round to round: `calls` back-to-back calls through the C ABI
on preallocated buffers, a host clock around them and a device synchronise at both ends (us per call).  Per variant: the
median over the rounds and the spread (max - min over the rounds) -- the run-to-run noise a difference has to exceed to mean
anything; with --parent, per pair of builds, whether the medians `agree` within the larger of the two spreads.  Before timing,
the outputs of the two libraries are compared bit for bit, and the weighted call with unit weights against the unweighted one.
Loss variants: `unweighted`, `weighted/mask` (30 % zeros, NaN measurements under them) and `weighted/null` (weights == NULL:
the weighted kernels on unit weights).  Metric variants: r2_metric_slices with R2_METRIC_SSIM along each axis, and with
R2_METRIC_SSIM | R2_METRIC_NORMALIZE along axis 0.  Prints one line per variant and one JSON line; exit status 1 if any bit
differs; nothing is asserted about the weighted cost."""
import argparse
import json
import statistics
import sys
import time

import torch

sys.path.insert(0, ".")
from r2_gaussian_amd import _lib
from r2_gaussian_amd._boundary import ptr_table


def time_rounds(variants, calls, rounds):
    """-> {variant: {median_us, min_us, max_us, spread_us}} of `calls` back-to-back calls, the variants alternating."""
    order = list(variants)
    times = {k: [] for k in order}
    for fn in variants.values():            # warm every variant at this shape
        for _ in range(50):
            fn()
    torch.cuda.synchronize()
    for r in range(rounds):
        for k in order[r % len(order):] + order[:r % len(order)]:
            fn = variants[k]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(calls):
                fn()
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) / calls * 1e6)
    return {k: {"median_us": statistics.median(ts), "min_us": min(ts), "max_us": max(ts), "spread_us": max(ts) - min(ts)}
            for k, ts in times.items()}


def report(result, group, recs, kinds, rounds, with_parent):
    """Prints and records a group's timings and, per kind, whether this build and the parent agree within the spread."""
    for k, rec in recs.items():
        result["variants"]["%s/%s" % (group, k)] = rec
        print("%-4s %-26s %8.2f us/call  (min %.2f, max %.2f, spread %.2f over %d rounds)" % (
            group, k, rec["median_us"], rec["min_us"], rec["max_us"], rec["spread_us"], rounds), flush=True)
    for kind in kinds if with_parent else ():
        a, b = recs[kind + "/this"], recs[kind + "/parent"]
        diff, noise = a["median_us"] - b["median_us"], max(a["spread_us"], b["spread_us"])
        result["%s/%s_agree" % (group, kind)] = bool(abs(diff) <= noise)
        result["%s/%s_this_minus_parent_us" % (group, kind)] = diff
        print("%-4s %s this - parent: difference of medians %+.2f us, run-to-run spread %.2f us: %s" % (
            group, kind, diff, noise, "agree" if abs(diff) <= noise else "DIFFER"), flush=True)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--parent", default=None, help="libr2hip.so of the build to compare this one against")
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--volume", type=int, nargs=3, default=(96, 128, 160), help="the metric's volume")
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
        libs["parent"] = _lib.bind(args.parent)
    n, lam = args.size, 0.25
    gen = torch.Generator().manual_seed(0)
    result = {"size": n, "volume": list(args.volume), "calls": args.calls, "rounds": args.rounds, "variants": {}}
    p = lambda t: t.data_ptr()
    tab = lambda t: ptr_table(list(t))

    def checked(fn):
        if fn() != 0:
            sys.exit("a call failed: %s" % here.r2_last_error())
        torch.cuda.synchronize()

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

        def unweighted(L):
            if V == 1:
                return lambda: L.r2_loss_l1_ssim(n, n, p(img), p(gt), 1.0, lam, p(grad), p(scratch), p(scalars), None)
            t = tab(gt)
            return lambda: L.r2_loss_l1_ssim_batch(V, n, n, p(img), t, 1.0, lam, p(grad), p(scratch), p(scalars), None)

        def weighted(L, y, wts):
            if V == 1:
                return lambda: L.r2_loss_l1_ssim_weighted(n, n, p(img), p(y), None if wts is None else p(wts), 1.0, lam, p(grad),
                                                          p(scratch), p(scalars), None)
            t, tw = tab(y), None if wts is None else tab(wts)
            return lambda: L.r2_loss_l1_ssim_weighted_batch(V, n, n, p(img), t, tw, 1.0, lam, p(grad), p(scratch), p(scalars), None)

        kinds = ("unweighted", "weighted/mask", "weighted/null")
        variants = {}
        for k, L in libs.items():
            variants["unweighted/" + k] = unweighted(L)
            variants["weighted/mask/" + k] = weighted(L, gt_nan, w)
            variants["weighted/null/" + k] = weighted(L, gt, None)

        rows = 1 if V == 1 else V + 1

        def outputs(fn, cols):
            grad.zero_()
            scalars.zero_()
            checked(fn)
            return grad.clone().view(torch.int32), scalars.clone().view(torch.int32)[:cols * rows].view(rows, cols)
        base_g, base_s = outputs(variants["unweighted/this"], 3)
        same = {}
        for name, fn in (("null", variants["weighted/null/this"]), ("ones", weighted(here, gt, ones))):
            g, s = outputs(fn, 4)
            same[name] = bool(torch.equal(g, base_g) and torch.equal(s[:, :3], base_s))
        for kind in kinds if "parent" in libs else ():
            cols = 3 if kind == "unweighted" else 4
            (g, s), (gp, sp) = outputs(variants[kind + "/this"], cols), outputs(variants[kind + "/parent"], cols)
            same[kind + "/parent"] = bool(torch.equal(g, gp) and torch.equal(s, sp))
        result["V%d/bits" % V] = same
        print("V %d  bit for bit (null, ones: against unweighted/this; */parent: this build against the parent): %s" % (V, same),
              flush=True)
        report(result, "V%d" % V, time_rounds(variants, args.calls, args.rounds), kinds, args.rounds, "parent" in libs)

    # ---- the per-slice metrics: the SSIM tile of the loss with a strided, scaled load
    n0, n1, n2 = args.volume
    vol = torch.rand((n0, n1, n2), generator=gen)
    pred = (vol + 0.05 * torch.randn((n0, n1, n2), generator=gen)).clamp_(min=0).to(dev)
    vol = vol.to(dev)
    per_slice = torch.empty((max(n0, n1, n2), 4), device=dev)
    mscratch = torch.empty(max(here.r2_metric_slices_scratch_floats(n0, n1, n2, a) for a in range(3)), device=dev)
    cases = {"ssim/axis%d" % a: (a, _lib.R2_METRIC_SSIM) for a in range(3)}
    cases["ssim+normalize/axis0"] = (0, _lib.R2_METRIC_SSIM | _lib.R2_METRIC_NORMALIZE)

    def metric(L, axis, flags):
        return lambda: L.r2_metric_slices(n0, n1, n2, axis, p(vol), p(pred), flags, p(per_slice), p(mscratch), None)

    variants = {"%s/%s" % (kind, k): metric(L, *case) for kind, case in cases.items() for k, L in libs.items()}

    def table(fn):
        per_slice.zero_()
        checked(fn)
        return per_slice.clone().view(torch.int32)
    if "parent" in libs:
        result["metric/bits"] = {kind: bool(torch.equal(table(variants[kind + "/this"]), table(variants[kind + "/parent"])))
                                 for kind in cases}
        print("metric  bit for bit, this build against the parent: %s" % result["metric/bits"], flush=True)
    report(result, "metric", time_rounds(variants, args.calls, args.rounds), list(cases), args.rounds, "parent" in libs)

    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    ok = all(v for k, v in result.items() if k.endswith("/bits") for v in v.values())
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
