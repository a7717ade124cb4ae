"""GPU: the trainer's opt-in neighbour smoothness term (train.training with opt.lambda_graph > 0): when the graph is built,
that the term stays finite across a densification, that the saved model loads -- and that with lambda_graph = 0 (the
default) graph.py is never called."""
import os

import numpy as np
import pytest
import torch

from tests import mini_trainer as T

pytestmark = pytest.mark.gpu
BOUND = (T.Opt.scale_min * 2.0, T.Opt.scale_max * 2.0)
ITERS, EVERY, DENSIFY_AT = 25, 10, 12


@pytest.fixture(scope="module")
def case():
    return T.Case(detector=128, n_vol=64, n_views=30, p_gt=6000, n_init=3000, seed=2)


def _train(case, path, **kw):
    from r2_gaussian_amd import train as TR
    # one densification, at iteration 12; a threshold every Gaussian passes, so that it changes P
    opt = TR.OptimizationParams(iterations=ITERS, position_lr_max_steps=ITERS, density_lr_max_steps=ITERS,
                                scaling_lr_max_steps=ITERS, rotation_lr_max_steps=ITERS, densify_from_iter=5,
                                densify_until_iter=20, densification_interval=DENSIFY_AT, densify_grad_threshold=1e-12, **kw)
    geo = dict(nVoxel=list(case.nVoxel), sVoxel=list(case.sVoxel), offOrigin=list(case.center), dVoxel=case.dVoxel.tolist())
    init = np.concatenate([case.init_xyz.numpy(), case.init_density.numpy()[:, None]], 1)
    return TR.training(case.views, [p.numpy() for p in case.projs], [], [], case.vol_gt.numpy(), geo, init, opt, str(path),
                       scale_bound=BOUND, seed=0, log=lambda *a: None)


def test_graph_term_across_a_densification(case, tmp_path, monkeypatch):
    from r2_gaussian_amd import graph as G
    from r2_gaussian_amd import model_io
    built, terms = [], []
    knn, smooth = G.knn_graph, G.graph_smoothness

    def knn_spy(xyz, k):
        assert not xyz.requires_grad and k == 4
        built.append(int(xyz.shape[0]))
        return knn(xyz, k)

    def smooth_spy(values, graph, **kw):
        assert kw == {"kind": "l1"} and values.shape == (graph.P,)
        t = smooth(values, graph, **kw)
        terms.append(t.detach())
        return t

    monkeypatch.setattr(G, "knn_graph", knn_spy)
    monkeypatch.setattr(G, "graph_smoothness", smooth_spy)
    out = _train(case, tmp_path / "on", lambda_graph=0.05, graph_k=4, graph_every=EVERY)
    assert len(terms) == ITERS and bool(torch.isfinite(torch.stack(terms)).all()) and float(torch.stack(terms).min()) > 0
    # a build at the first iteration, at every graph_every boundary, and at the iteration after the densification changed P
    boundaries = ITERS // EVERY
    p_changes = sum(a != b for a, b in zip(built, built[1:]))
    print("builds at P =", built, "final P", out["P"])
    assert out["P"] != 3000 and p_changes == 1
    assert out["graph_builds"] == len(built) == 1 + boundaries + p_changes
    assert built == [3000, 3000, out["P"], out["P"]]
    m = model_io.load_point_cloud(os.path.join(str(tmp_path / "on"), "point_cloud", "iteration_%d" % ITERS, "point_cloud.pickle"))
    assert m["xyz"].shape == (out["P"], 3) and m["density"].shape == (out["P"], 1)
    assert all(bool(torch.isfinite(torch.as_tensor(m[k])).all()) for k in ("xyz", "density", "scaling", "rotation"))


def test_off_by_default_never_calls_the_graph_module(case, tmp_path, monkeypatch):
    from r2_gaussian_amd import graph as G

    def boom(*a, **k):
        raise AssertionError("graph.py called with lambda_graph = 0")

    monkeypatch.setattr(G, "knn_graph", boom)
    monkeypatch.setattr(G, "graph_smoothness", boom)
    out = _train(case, tmp_path / "off")
    assert out["graph_builds"] == 0 and out["P"] != 3000

    class Bare:   # an opt object from before the new keywords: read with their defaults
        pass

    from r2_gaussian_amd import train as TR
    bare = Bare()
    for k, v in vars(TR.OptimizationParams).items():
        if not k.startswith("_") and k not in ("lambda_graph", "graph_k", "graph_every"):
            setattr(bare, k, v)
    bare.iterations = 2
    geo = dict(nVoxel=list(case.nVoxel), sVoxel=list(case.sVoxel), offOrigin=list(case.center), dVoxel=case.dVoxel.tolist())
    init = np.concatenate([case.init_xyz.numpy(), case.init_density.numpy()[:, None]], 1)
    out = TR.training(case.views, [p.numpy() for p in case.projs], [], [], case.vol_gt.numpy(), geo, init, bare,
                      str(tmp_path / "bare"), scale_bound=BOUND, seed=0, log=lambda *a: None)
    assert out["graph_builds"] == 0
