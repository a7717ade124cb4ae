"""What do the neighbour graph and the smoothness loss cost?  ("Neighbour graphs and the smoothness loss".)

    python scripts/graph_bench.py [--P 50000 300000] [--K 3 8 16] [--reps 20] [--out graph_bench.json]

On scene.make_cloud clouds, in one process:

* ``graph.knn_graph`` (search + transpose) for every P and K, its search alone (r2_knn_graph), an independent baseline --
  chunked ``torch.cdist`` + ``topk`` -- and, for K = 3, ``distCUDA2`` (the same search without the indices);
* ``graph.graph_smoothness`` forward + backward for every kind against a torch formulation of the same sum (``gather`` for
  the forward, autograd's ``index_add_`` for the backward), and the largest difference of their gradients;
* a training iteration of the native model at the first P (512^2 view, fused image loss, 32^3 TV patch, statistics, step:
  scripts/train_bench.py's) with and without the graph term (graph already built), the two alternating.

Times: the protocol of scripts/plan_bench.py -- one pair of HIP events around every call after three warm-up calls, the median
over `reps` calls with the smallest and the largest.  One process, one run.  Not a test and not a gate.
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from r2_gaussian_amd import _lib                                                             # noqa: E402
from r2_gaussian_amd import distCUDA2                                                        # noqa: E402
from r2_gaussian_amd import graph as G                                                       # noqa: E402
from r2_gaussian_amd import scene as S                                                       # noqa: E402
from r2_gaussian_amd._C import _stream                                                       # noqa: E402
from scripts.field_error import timed                                                        # noqa: E402
from scripts.plan_bench import timed_pair                                                    # noqa: E402


def cdist_topk(pts, K, chunk=4096):
    """The K nearest by torch alone: rows of cdist in chunks, self masked by index, topk.  (Not bit-comparable: cdist forms
    distances through a matrix product.)"""
    P = pts.shape[0]
    idx = torch.empty((P, K), dtype=torch.int64, device=pts.device)
    for a in range(0, P, chunk):
        d = torch.cdist(pts[a:a + chunk], pts)
        n = d.shape[0]
        d[torch.arange(n, device=pts.device), torch.arange(a, a + n, device=pts.device)] = float("inf")
        idx[a:a + n] = d.topk(K, dim=1, largest=False).indices
    return idx


def search_only(pts, K):
    L = _lib.lib()
    P = pts.shape[0]
    idx = torch.empty((P, K), dtype=torch.int32, device=pts.device)
    d2 = torch.empty((P, K), dtype=torch.float32, device=pts.device)
    nbytes = int(L.r2_knn_graph_workspace_bytes(P, K))
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=pts.device)
    _lib.check(L.r2_knn_graph(P, pts.data_ptr(), K, idx.data_ptr(), d2.data_ptr(), ws.data_ptr(), nbytes, _stream(pts.device)),
               "r2_knn_graph")
    return idx


def torch_smoothness(v, idx, kind, delta, scale):
    x = v[:, None] - v[idx.long()]
    if kind == "l1":
        t = x.abs()
    elif kind == "l2":
        t = x * x
    else:
        t = torch.where(x.abs() <= delta, 0.5 * x * x, delta * (x.abs() - 0.5 * delta))
    return scale * t.sum()


def make_iteration(model, views, gts, graph, lam):
    """scripts/train_bench.py's native iteration, plus lam * graph_smoothness when lam > 0."""
    from r2_gaussian_amd import GaussianRasterizer
    from r2_gaussian_amd import losses as FL
    from r2_gaussian_amd.train import _query, _settings
    dev = torch.device("cuda:0")
    settings = [_settings(v, dev) for v in views]
    centre = torch.zeros(3)
    tvN = torch.tensor([32, 32, 32])
    tvS = torch.tensor([2.0 / 256] * 3) * tvN
    state = {"it": 1}

    def iteration():
        it = state["it"]
        state["it"] += 1
        x, d, s, r = model.activated()
        screen = torch.zeros_like(x, requires_grad=True)
        img, radii = GaussianRasterizer(settings[it % len(views)])(x, screen, d, scales=s, rotations=r)
        loss, _ = FL.image_loss(img, gts[it % len(views)], 0.25)
        loss = loss + 0.05 * FL.tv_3d_loss(_query(x, d, s, r, centre, tvN, tvS))
        if lam > 0:
            loss = loss + lam * G.graph_smoothness(d[:, 0], graph, kind="l1")
        loss.backward()
        with torch.no_grad():
            model.add_densification_stats(radii, screen.grad)
            model.step(it)
    return iteration


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--P", type=int, nargs="+", default=[50000, 300000])
    ap.add_argument("--K", type=int, nargs="+", default=[3, 8, 16])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default="", help="also write the results to this JSON file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("graph_bench.py measures on the GPU: none visible")
    dev = torch.device("cuda:0")
    res = {}

    def emit(key, value):
        res[key] = value
        print(key, json.dumps(value))
        sys.stdout.flush()

    for P in a.P:
        cloud = S.make_cloud(P, seed=7)
        pts = cloud.xyz.to(dev).contiguous()
        for K in a.K:
            g = G.knn_graph(pts, K)
            base = cdist_topk(pts, K)
            # (same neighbour SETS wherever cdist's distances do not reorder near-ties: reported, not asserted)
            agree = float((torch.sort(g.idx.long(), 1).values == torch.sort(base, 1).values).all(1).float().mean())
            row = {"knn_graph": timed(lambda: G.knn_graph(pts, K), a.reps, dev),
                   "search_only": timed(lambda: search_only(pts, K), a.reps, dev),
                   "cdist_topk": timed(lambda: cdist_topk(pts, K), 3, dev, warm=1),
                   "rows_equal_to_cdist_topk": agree}
            if K == 3:
                row["distCUDA2"] = timed(lambda: distCUDA2(pts), a.reps, dev)
            emit("knn_P%d_K%d" % (P, K), row)
            if K != 8:
                continue
            v = cloud.density.reshape(-1).to(dev)
            scale = 1.0 / g.n_edges
            for kind in ("l1", "l2", "huber"):
                delta = 0.1 if kind == "huber" else None
                x = v.clone().requires_grad_(True)
                y = v.clone().requires_grad_(True)

                def ours():
                    x.grad = None
                    G.graph_smoothness(x, g, kind=kind, delta=delta).backward()

                def theirs():
                    y.grad = None
                    torch_smoothness(y, g.idx, kind, delta, scale).backward()

                ours()
                theirs()
                r = timed_pair(ours, theirs, a.reps, dev)
                r = {"hip": r["planned"], "torch": r["unplanned"], "ratio": r["ratio"], "separate": r["separate"],
                     "max_grad_difference": float((x.grad - y.grad).abs().max()), "max_grad": float(y.grad.abs().max())}
                emit("loss_P%d_K8_%s" % (P, kind), r)

    # a training iteration with and without the term
    from r2_gaussian_amd.gaussians import GaussianModel
    from r2_gaussian_amd.train import OptimizationParams
    P = a.P[0]
    cloud = S.make_cloud(P, seed=0)
    views = S.make_views(8, (512, 512))
    gen = torch.Generator().manual_seed(1)
    gts = [torch.rand((1, 512, 512), generator=gen).to(dev) * 0.5 for _ in views]
    legs = {}
    for name, lam in (("with", 0.01), ("without", 0.0)):
        m = GaussianModel((0.0005 * 2.0, 0.5 * 2.0), device=dev)
        m.create_from_pcd(cloud.xyz.numpy(), cloud.density.reshape(-1, 1).numpy(), 1.0)
        m.training_setup(OptimizationParams())
        graph = G.knn_graph(m.activated()[0].detach(), 8) if lam > 0 else None
        legs[name] = make_iteration(m, views, gts, graph, lam)
    r = timed_pair(legs["with"], legs["without"], a.reps, dev, warm=10)
    emit("train_iteration_P%d_K8" % P, {"with_graph_term": r["planned"], "without": r["unplanned"], "ratio": r["ratio"],
                                        "separate": r["separate"]})
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
