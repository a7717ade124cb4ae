"""What does merging neighbouring Gaussians cost, how much does it merge, and how far does it move the cloud's images?
("Merging neighbouring Gaussians".)

    python scripts/merge_bench.py [--P 50000 300000] [--trained large] [--K 8] [--reps 20] [--out merge_bench.json]

On scene.make_cloud clouds and, where tests/trained_cloud.py can load or train one, a trained densified cloud, in one process:

* times of ``merge.merge_costs``, ``merge.match_edges`` (12 rounds) and ``merge.merge_pairs`` (count + emit, one host read) next
  to ``graph.knn_graph`` at the same K;
* for max_cost in {0.05, 0.1, 0.25, 0.5}: pairs, open after 12 rounds, the rounds after which nothing is open (doubling the
  rounds until open = 0; every probe is a full count, so this is not timed), P after;
* the relative RMS and the largest change, relative to the largest value, of ``project_gaussians`` on 8 views (256^2) and of
  ``query_points`` on a 64^3 grid over [-1, 1]^3 between the cloud before and after.

Times: one pair of HIP events around every call after three warm-up calls, the median over `reps` calls with the smallest and
the largest (scripts/field_error.timed).  One process, one run.  Not a test and not a gate.
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from r2_gaussian_amd import graph as G                                                       # noqa: E402
from r2_gaussian_amd import merge as MG                                                      # noqa: E402
from r2_gaussian_amd import scene as S                                                       # noqa: E402
from r2_gaussian_amd.field import query_points                                               # noqa: E402
from r2_gaussian_amd.gaussian_projector import project_gaussians                             # noqa: E402
from scripts.field_error import timed                                                        # noqa: E402

MAX_COSTS = (0.05, 0.1, 0.25, 0.5)


def change(before, after):
    d = (after - before).double()
    ref = before.double()
    return {"rel_rms": float(d.pow(2).mean().sqrt() / ref.pow(2).mean().sqrt()), "rel_max": float(d.abs().max() / ref.abs().max())}


def rounds_to_maximal(g, cost, max_cost, params, limit=256):
    """The smallest number of rounds among 1, 2, 4, ... and the exact one below it (bisection) after which nothing is open."""
    def n_open(r):
        return MG.merge_pairs(g, cost, max_cost, MG.match_edges(g, cost, max_cost, rounds=r), *params)[5]["open"]
    hi = 1
    while hi < limit and n_open(hi) > 0:
        hi *= 2
    lo = hi // 2
    while lo + 1 < hi:
        mid = (lo + hi) // 2
        if n_open(mid) > 0:
            lo = mid
        else:
            hi = mid
    return hi


def bench_cloud(name, cloud, K, reps, dev, emit):
    params = [t.to(dev).contiguous() for t in (cloud.xyz, cloud.density, cloud.scales, cloud.rotations)]
    P = params[0].shape[0]
    g = G.knn_graph(params[0], K)
    cost = MG.merge_costs(g, *params)
    mate = MG.match_edges(g, cost, 0.1, rounds=12)
    fin = cost[torch.isfinite(cost)]
    q = torch.quantile(fin[:: max(1, fin.numel() // 1000000)].double(), torch.tensor([0.01, 0.1, 0.5, 0.9], dtype=torch.float64, device=dev))
    emit("time_%s" % name, {"P": P, "K": K,
                            "knn_graph": timed(lambda: G.knn_graph(params[0], K), reps, dev),
                            "merge_costs": timed(lambda: MG.merge_costs(g, *params), reps, dev),
                            "match_edges_12_rounds": timed(lambda: MG.match_edges(g, cost, 0.1, rounds=12), reps, dev),
                            "merge_pairs_count_emit": timed(lambda: MG.merge_pairs(g, cost, 0.1, mate, *params), reps, dev),
                            "merge_gaussians_all": timed(lambda: MG.merge_gaussians(*params, max_cost=0.1, k=K), reps, dev),
                            "cost_quantiles_1_10_50_90": [float(v) for v in q]})
    views = S.make_views(8, (256, 256))
    lin = torch.linspace(-1.0, 1.0, 64, device=dev)
    grid = torch.stack(torch.meshgrid(lin, lin, lin, indexing="ij"), -1).contiguous()
    with torch.no_grad():
        proj0 = project_gaussians(views, *params)
        field0 = query_points(grid, *params)
        for max_cost in MAX_COSTS:
            out = MG.merge_gaussians(*params, max_cost=max_cost, k=K, graph=g)
            row = {"P": P, "pairs": out[5]["pairs"], "open_after_12_rounds": out[5]["open"], "P_after": out[5]["P"],
                   "rounds_to_open_0": rounds_to_maximal(g, cost, max_cost, params),
                   "projection": change(proj0, project_gaussians(views, *out[:4])),
                   "field": change(field0, query_points(grid, *out[:4]))}
            mass0 = (params[1][:, 0].double() * params[2].double().prod(1)).sum()
            mass1 = (out[1][:, 0].double() * out[2].double().prod(1)).sum()
            row["total_mass_rel_change"] = float((mass1 - mass0).abs() / mass0)
            emit("merge_%s_cost%g" % (name, max_cost), row)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--P", type=int, nargs="*", default=[50000, 300000])
    ap.add_argument("--trained", default="large", help="tests/trained_cloud.py name ('' = none)")
    ap.add_argument("--K", type=int, default=8)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default="", help="also write the results to this JSON file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("merge_bench.py measures on the GPU: none visible")
    dev = torch.device("cuda:0")
    res = {}

    def emit(key, value):
        res[key] = value
        print(key, json.dumps(value))
        sys.stdout.flush()
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                json.dump(res, f, indent=1)

    for P in a.P:
        bench_cloud("synthetic%dk" % (P // 1000), S.make_cloud(P, seed=7), a.K, a.reps, dev, emit)
    if a.trained:
        try:
            from tests import trained_cloud as TC
            cloud, info = TC.load(a.trained)
        except Exception as e:   # no trained cloud on this machine: say so, measure nothing
            cloud = None
            emit("trained_%s" % a.trained, {"not_measured": repr(e)})
        if cloud is not None:
            bench_cloud("trained_%s" % a.trained, cloud, a.K, a.reps, dev, emit)


if __name__ == "__main__":
    main()
