"""GPU: the trainer's opt-in merging (train.training with opt.merge_interval > 0) on the smallest case
tests/test_train_views_gpu.py trains: P drops at the merge iteration against a twin run without it, the run stays finite and
is the same on a second run, and with merge_interval = 0 (the default) the loop is the one it was, bit for bit.  No PSNR
threshold: what merging does to quality is what scripts/merge_bench.py reports."""
import numpy as np
import pytest
import torch

from tests import mini_trainer as T

pytestmark = pytest.mark.gpu
BOUND = (T.Opt.scale_min * 2.0, T.Opt.scale_max * 2.0)
ITERS, DENSIFY_AT, MERGE_AT = 40, 15, 30


@pytest.fixture(scope="module")
def case():
    return T.Case(detector=64, n_vol=32, n_views=10, p_gt=2000, n_init=1500, seed=2)


def _args(case):
    geo = dict(nVoxel=list(case.nVoxel), sVoxel=list(case.sVoxel), offOrigin=list(case.center), dVoxel=case.dVoxel.tolist())
    init = np.concatenate([case.init_xyz.numpy(), case.init_density.numpy()[:, None]], 1)
    return (case.views, [p.numpy() for p in case.projs], [], [], case.vol_gt.numpy(), geo, init)


def _opt(**kw):
    from r2_gaussian_amd import train as TR
    # one densification at iteration 15 with a threshold every Gaussian passes (clones sit on their originals: mergeable)
    return TR.OptimizationParams(iterations=ITERS, position_lr_max_steps=ITERS, density_lr_max_steps=ITERS,
                                 scaling_lr_max_steps=ITERS, rotation_lr_max_steps=ITERS, densify_from_iter=5,
                                 densify_until_iter=20, densification_interval=DENSIFY_AT, densify_grad_threshold=1e-12, **kw)


def _train(case, path, opt):
    from r2_gaussian_amd import train as TR
    return TR.training(*_args(case), opt, str(path), scale_bound=BOUND, seed=0, log=lambda *a: None)


@pytest.fixture(scope="module")
def twin(case, tmp_path_factory):
    """The run without merging, shared by the tests; never modified."""
    return _train(case, tmp_path_factory.mktemp("twin"), _opt())


def test_merging_lowers_P_and_is_deterministic(case, twin, tmp_path, monkeypatch):
    from r2_gaussian_amd.gaussians import NAMES, GaussianModel
    calls = []
    merge = GaussianModel.merge

    def spy(self, max_cost, k=8, rounds=12):
        before = self.P
        pairs = merge(self, max_cost, k=k, rounds=rounds)
        calls.append((before, self.P, pairs, max_cost, k))
        return pairs

    monkeypatch.setattr(GaussianModel, "merge", spy)
    kw = dict(merge_interval=MERGE_AT, merge_cost=0.25, merge_k=4, merge_from_iter=20, merge_until_iter=35)
    one = _train(case, tmp_path / "a", _opt(**kw))
    two = _train(case, tmp_path / "b", _opt(**kw))
    print("P without merging %d, with %d; merge calls %s" % (twin["P"], one["P"], calls))
    # exactly one call per run, at iteration 30, after the densification of iteration 15 had grown the cloud
    assert len(calls) == 2 and calls[0] == calls[1]
    before, after, pairs, max_cost, k = calls[0]
    assert before == twin["P"] and (max_cost, k) == (0.25, 4)
    assert pairs > 0 and after == before - pairs and one["merged_pairs"] == pairs
    assert one["P"] == after < twin["P"]
    m = one["model"]
    for n in NAMES:
        assert bool(torch.isfinite(m._raw[n]).all()), n
        assert torch.equal(m._raw[n], two["model"]._raw[n]), n                      # the same bits on a second run
        assert torch.equal(m.exp_avg[n], two["model"].exp_avg[n]) and m.exp_avg[n].shape[0] == after
    assert all(bool(torch.isfinite(a).all()) for a in m.activated())
    assert m.denom.shape == (after, 1) and 0 < float(m.denom.max()) <= ITERS - MERGE_AT   # the merge reset the statistics
    # the interval alone does not merge outside (merge_from_iter, merge_until_iter)
    calls.clear()
    out = _train(case, tmp_path / "c", _opt(merge_interval=MERGE_AT, merge_from_iter=30, merge_until_iter=40))
    assert calls == [] and out["merged_pairs"] == 0 and out["P"] == twin["P"]


def test_off_by_default_is_the_loop_as_it_was(case, twin, tmp_path, monkeypatch):
    from r2_gaussian_amd import train as TR
    from r2_gaussian_amd.gaussians import NAMES, GaussianModel

    def boom(*a, **k):
        raise AssertionError("GaussianModel.merge called with merge_interval = 0")

    monkeypatch.setattr(GaussianModel, "merge", boom)

    class Bare:   # an opt object from before the new keywords: no merge_* attribute at all
        pass

    bare = Bare()
    for k, v in vars(_opt()).items():
        setattr(bare, k, v)
    for k, v in vars(TR.OptimizationParams).items():
        if not k.startswith("_") and not k.startswith("merge_") and not hasattr(bare, k):
            setattr(bare, k, v)
    assert not any(hasattr(bare, k) for k in ("merge_interval", "merge_cost", "merge_k", "merge_from_iter", "merge_until_iter"))
    old = _train(case, tmp_path / "bare", bare)
    assert old["merged_pairs"] == 0 and old["P"] == twin["P"] != 1500
    for n in NAMES:
        assert torch.equal(old["model"]._raw[n], twin["model"]._raw[n]), n
        assert torch.equal(old["model"].exp_avg[n], twin["model"].exp_avg[n]), n
    with pytest.raises(ValueError):
        _train(case, tmp_path / "neg", _opt(merge_interval=-1))
