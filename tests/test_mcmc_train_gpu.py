"""GPU: the trainer's opt-in fixed-budget strategy (train.training with opt.densify_strategy = "mcmc") on the case and shape of
tests/test_merge_train_gpu.py: the densification slot relocates instead of densifying and grows the cloud by 5 % under the cap,
every step is followed by the position noise, the run stays finite and is the same on a second run; with the default strategy
-- and an opt object from before the new fields -- the loop is the one it was, bit for bit.  No PSNR threshold: what the
strategy does to quality is what scripts/mcmc_bench.py reports."""
import math

import numpy as np
import pytest
import torch

from tests import mini_trainer as T

pytestmark = pytest.mark.gpu
BOUND = (T.Opt.scale_min * 2.0, T.Opt.scale_max * 2.0)
ITERS, SLOT, N_INIT, CAP = 40, 15, 1500, 1700
NEW_FIELDS = ("densify_strategy", "dead_density", "cap_max", "lambda_density_l1", "lambda_scale_l1")


@pytest.fixture(scope="module")
def case():
    return T.Case(detector=64, n_vol=32, n_views=10, p_gt=2000, n_init=N_INIT, seed=2)


def _args(case):
    geo = dict(nVoxel=list(case.nVoxel), sVoxel=list(case.sVoxel), offOrigin=list(case.center), dVoxel=case.dVoxel.tolist())
    init = np.concatenate([case.init_xyz.numpy(), case.init_density.numpy()[:, None]], 1)
    return (case.views, [p.numpy() for p in case.projs], [], [], case.vol_gt.numpy(), geo, init)


def _opt(**kw):
    from r2_gaussian_amd import train as TR
    # one densification slot, at iteration 15
    return TR.OptimizationParams(iterations=ITERS, position_lr_max_steps=ITERS, density_lr_max_steps=ITERS,
                                 scaling_lr_max_steps=ITERS, rotation_lr_max_steps=ITERS, densify_from_iter=5,
                                 densify_until_iter=20, densification_interval=SLOT, densify_grad_threshold=1e-12, **kw)


def _train(case, path, opt):
    from r2_gaussian_amd import train as TR
    return TR.training(*_args(case), opt, str(path), scale_bound=BOUND, seed=0, log=lambda *a: None)


def test_mcmc_strategy_keeps_the_budget_and_is_deterministic(case, tmp_path, monkeypatch):
    from r2_gaussian_amd.gaussians import NAMES, GaussianModel
    log = []
    relocate, add_noise = GaussianModel.relocate, GaussianModel.add_noise

    def spy_relocate(self, call, dead_density, cap_max, **kw):
        before = self.P
        n = relocate(self, call, dead_density, cap_max, **kw)
        assert self.P <= cap_max
        log.append(("relocate", call, before, self.P, n, dead_density, cap_max))
        return n

    def spy_noise(self, call, *a, **kw):
        log.append(("noise", call, self.steps["xyz"]))
        return add_noise(self, call, *a, **kw)

    def boom(*a, **k):
        raise AssertionError("densify_and_prune called with densify_strategy = 'mcmc'")

    monkeypatch.setattr(GaussianModel, "relocate", spy_relocate)
    monkeypatch.setattr(GaussianModel, "add_noise", spy_noise)
    monkeypatch.setattr(GaussianModel, "densify_and_prune", boom)
    one = _train(case, tmp_path / "a", _opt(densify_strategy="mcmc", cap_max=CAP))
    first = list(log)
    log.clear()
    two = _train(case, tmp_path / "b", _opt(densify_strategy="mcmc", cap_max=CAP))
    assert log == first
    want = min(CAP, math.ceil(1.05 * N_INIT))
    assert [e for e in first if e[0] == "relocate"] == [("relocate", SLOT, N_INIT, want, want - N_INIT, 0.005, CAP)]
    # the noise follows every step(): iterations 1 .. ITERS - 1 (the last iteration takes no step), once each.  The step of
    # the relocation's own iteration finds new leaves without gradients and moves nothing, as after a densification: the
    # step count of xyz stays behind by one from there on
    assert [e[1:] for e in first if e[0] == "noise"] == [(it, it if it < SLOT else it - 1) for it in range(1, ITERS)]
    assert one["P"] == want <= CAP and one["relocations"] == 1
    m = one["model"]
    for n in NAMES:
        assert bool(torch.isfinite(m._raw[n]).all()), n
        assert torch.equal(m._raw[n], two["model"]._raw[n]), n                      # the same bits on a second run
        assert torch.equal(m.exp_avg[n], two["model"].exp_avg[n]) and m.exp_avg[n].shape[0] == want
        assert torch.equal(m.exp_avg_sq[n], two["model"].exp_avg_sq[n])
    assert all(bool(torch.isfinite(a).all()) for a in m.activated())
    assert m.denom.shape == (want, 1) and m.max_radii2D.shape == (want,)
    # a cap below the 5 %: the cloud stops there
    log.clear()
    out = _train(case, tmp_path / "c", _opt(densify_strategy="mcmc", cap_max=N_INIT + 10))
    assert out["P"] == N_INIT + 10 and [e[4] for e in log if e[0] == "relocate"] == [10]
    with pytest.raises(ValueError):
        _train(case, tmp_path / "d", _opt(densify_strategy="langevin"))


def test_default_strategy_is_the_loop_as_it_was(case, tmp_path, monkeypatch):
    from r2_gaussian_amd import train as TR
    from r2_gaussian_amd.gaussians import NAMES, GaussianModel
    twin = _train(case, tmp_path / "twin", _opt())

    def boom(*a, **k):
        raise AssertionError("the fixed-budget strategy ran with densify_strategy = 'threshold'")

    monkeypatch.setattr(GaussianModel, "relocate", boom)
    monkeypatch.setattr(GaussianModel, "add_noise", boom)

    class Bare:   # an opt object from before the new fields: none of them at all
        pass

    bare = Bare()
    for k, v in vars(_opt()).items():
        setattr(bare, k, v)
    for k, v in vars(TR.OptimizationParams).items():
        if not k.startswith("_") and k not in NEW_FIELDS and not hasattr(bare, k):
            setattr(bare, k, v)
    assert not any(hasattr(bare, k) for k in NEW_FIELDS)
    old = _train(case, tmp_path / "bare", bare)
    assert old["relocations"] == 0 and old["P"] == twin["P"] != N_INIT
    for n in NAMES:
        assert torch.equal(old["model"]._raw[n], twin["model"]._raw[n]), n
        assert torch.equal(old["model"].exp_avg[n], twin["model"].exp_avg[n]), n
        assert torch.equal(old["model"].exp_avg_sq[n], twin["model"].exp_avg_sq[n]), n
