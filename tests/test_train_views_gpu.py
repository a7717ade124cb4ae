"""GPU: several views per optimiser step in the native trainer (train.training(views_per_step=W), --views_per_step): one step
against the same step composed from the single-view pieces, W = 1 against the loop without the argument, 600 steps at W = 4
against tests/mini_trainer.py, and the command line."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import yaml

from tests import mini_trainer as T

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUND = (T.Opt.scale_min * 2.0, T.Opt.scale_max * 2.0)


def _geo(case):
    return dict(nVoxel=list(case.nVoxel), sVoxel=list(case.sVoxel), offOrigin=list(case.center), dVoxel=case.dVoxel.tolist())


def _init(case):
    return np.concatenate([case.init_xyz.numpy(), case.init_density.numpy()[:, None]], 1)


def _opt(TR, iters, **kw):
    return TR.OptimizationParams(iterations=iters, position_lr_max_steps=iters, density_lr_max_steps=iters,
                                 scaling_lr_max_steps=iters, rotation_lr_max_steps=iters, **kw)


def _close(a, b, scale=None):
    """The tolerance tests/test_batch_gpu.py:122 applies to batched-versus-single gradients -> the largest fraction of it."""
    scale = float(b.abs().max()) if scale is None else scale
    err, tol = (a - b).abs(), 1e-5 * b.abs() + 1e-6 * scale
    return float(torch.where(err == 0, torch.zeros_like(err), err / tol).max())


def test_one_step_of_four_views_against_the_single_view_pieces(gpu):
    """Both models take one step on the same four views.  Batched: train.render_loss_batch (one GaussianRasterizerBatch call,
    one image_loss_batch node), one batched statistics call.  Composed: four GaussianRasterizer calls, four image_loss nodes,
    their mean, four add_densification_stats calls.  Both add the same TV term.  The composed reference's screen-space
    gradients carry the mean's 1 / 4 as well, so the statistics are compared at grad_scale = 1, bit for bit (1 / 4 is a power
    of two: the loss kernels' weights / 4 and the upstream gradient 1 / 4 scale every product exactly)."""
    from r2_gaussian_amd import GaussianRasterizer
    from r2_gaussian_amd import losses as FL
    from r2_gaussian_amd import train as TR
    from r2_gaussian_amd.densify import densification_stats_batch
    from r2_gaussian_amd.gaussians import NAMES, GaussianModel
    case = T.Case(detector=128, n_vol=64, n_views=30, p_gt=6000, n_init=3000, seed=2)
    opt = _opt(TR, 100)
    picked = [3, 17, 8, 26]
    views = [case.views[i] for i in picked]
    gts = [case.projs[i].to(gpu) for i in picked]
    tvN = torch.tensor([opt.tv_vol_size] * 3)
    tvS = case.dVoxel * tvN
    centre = torch.tensor([0.1, -0.2, 0.05])
    models = []
    for _ in range(2):
        m = GaussianModel(BOUND, device=gpu)
        m.create_from_pcd(case.init_xyz.numpy(), case.init_density.numpy()[:, None], 1.0)
        # anisotropic, rotated Gaussians: the initial ones (equal scales, identity rotation) have no rotation gradient
        g = torch.Generator().manual_seed(3)
        m._set(m._raw["xyz"], m._raw["density"], m._raw["scaling"].cpu() + 0.3 * torch.randn(m.P, 3, generator=g),
               m._raw["rotation"].cpu() + 0.3 * torch.randn(m.P, 4, generator=g))
        m.training_setup(opt)
        m.update_learning_rate(1)
        models.append(m)
    a, b = models
    before = {n: a._raw[n].detach().clone() for n in NAMES}

    def tv(m):
        return opt.lambda_tv * FL.tv_3d_loss(TR._query(*m.activated(), centre, tvN, tvS))

    # batched
    loss_img, radii, screen = TR.render_loss_batch(a, views, gts, opt.lambda_dssim, gpu)
    loss_a = loss_img + tv(a)
    loss_a.backward()
    grads_a = [t.grad.clone() for t in a.activated()]
    zeros = [torch.zeros_like(t) for t in (a.max_radii2D, a.xyz_gradient_accum, a.denom)]
    scaled = [t.clone() for t in zeros]
    densification_stats_batch(radii, screen.grad, *scaled, grad_scale=4.0)        # the trainer's own call: grad_scale = W
    a.add_densification_stats(radii, screen.grad, grad_scale=1.0)
    # composed
    xyz, dens, scal, rot = b.activated()
    losses, per_view = [], []
    for v, gt in zip(views, gts):
        s = torch.zeros_like(xyz, requires_grad=True)
        img, r = GaussianRasterizer(raster_settings=TR._settings(v, gpu))(means3D=xyz, means2D=s, opacities=dens, scales=scal,
                                                                          rotations=rot, cov3D_precomp=None)
        losses.append(FL.image_loss(img, gt, opt.lambda_dssim)[0])
        per_view.append((r, s))
    loss_b = torch.stack(losses).mean() + tv(b)
    loss_b.backward()
    grads_b = [t.grad.clone() for t in b.activated()]
    for r, s in per_view:
        b.add_densification_stats(r, s.grad)
    torch.cuda.synchronize()

    assert bool((a.denom > 0).any()) and bool((a.xyz_gradient_accum > 0).any())
    for n in ("max_radii2D", "xyz_gradient_accum", "denom"):
        assert torch.equal(getattr(a, n), getattr(b, n)), n
    assert torch.equal(scaled[1], 4.0 * a.xyz_gradient_accum)          # from zero statistics: the value is the increment
    assert torch.equal(scaled[0], a.max_radii2D) and torch.equal(scaled[2], a.denom)
    frac = {"loss": _close(loss_a.detach(), loss_b.detach())}
    for n, ga, gb in zip(NAMES, grads_a, grads_b):
        frac["grad " + n] = _close(ga, gb)
    print("fractions of rtol 1e-5 / atol 1e-6 max|.|:", frac)
    assert all(f <= 1.0 for f in frac.values()), frac

    a.step()
    b.step()
    torch.cuda.synchronize()
    # the raw parameters: the same tolerance on the steps taken in units of the learning rate, i.e. on (p - p_before) / lr,
    # whose entries are at most 1 in magnitude for Adam
    step_frac = {}
    for n in NAMES:
        ua, ub = (a._raw[n].detach() - before[n]) / a.lr[n], (b._raw[n].detach() - before[n]) / b.lr[n]
        assert float(ub.abs().max()) > 0.5, n                           # the step moved the parameters
        step_frac[n] = _close(ua, ub)
    print("raw parameters, fractions of the tolerance x lr:", step_frac)
    assert all(f <= 1.0 for f in step_frac.values()), step_frac


def test_one_view_per_step_is_the_loop_as_it_was(tmp_path, gpu):
    from r2_gaussian_amd import train as TR
    from r2_gaussian_amd.gaussians import NAMES
    case = T.Case(detector=64, n_vol=32, n_views=10, p_gt=2000, n_init=1500, seed=2)
    opt = _opt(TR, 60, densify_from_iter=20, densify_until_iter=50, densification_interval=30)
    kw = dict(scale_bound=BOUND, seed=0, log=lambda *a: None)
    args = (case.views, [p.numpy() for p in case.projs], [], [], case.vol_gt.numpy(), _geo(case), _init(case), opt)
    one = TR.training(*args, str(tmp_path / "a"), views_per_step=1, **kw)
    two = TR.training(*args, str(tmp_path / "b"), **kw)
    print("P %d -> %d" % (case.init_xyz.shape[0], one["P"]))
    assert one["P"] == two["P"]
    assert 0 < float(one["model"].denom.max()) <= 30          # the densification at iteration 30 reset the statistics
    for n in NAMES:
        assert torch.equal(one["model"]._raw[n], two["model"]._raw[n]), n
    with pytest.raises(ValueError):
        TR.training(*args, str(tmp_path / "c"), views_per_step=0, **kw)


def test_loop_of_four_views_matches_mini_trainer(tmp_path, gpu):
    """test_train_gpu.py::test_loop_matches_mini_trainer at W = 4: 600 optimiser steps of four views end within 0.2 dB of 3D
    PSNR of mini_trainer.train(views_per_step=4) (torch Adam, one render per view, statistics from every view's own gradient)
    with the same options and seed: both draw the same views, TV centres and split samples.  Measured on an MI355X: native
    27.587 dB (P 17176), mini_trainer 27.586 dB (P 17175), from 19.645 dB."""
    from r2_gaussian_amd import train as TR
    from r2_gaussian_amd import scene as S
    iters = 600
    kw = dict(iterations=iters, densify_from_iter=150, densify_until_iter=500, densification_interval=100)
    case = T.Case(detector=128, n_vol=64, n_views=30, p_gt=8000, n_init=3000, seed=2)
    ref = T.train(case, T.Opt(**kw), "hip", eval_every=iters, seed=0, fused_losses=True, fused_densify=True, views_per_step=4)
    del kw["iterations"]
    out = TR.training(case.views, [p.numpy() for p in case.projs], [], [], case.vol_gt.numpy(), _geo(case), _init(case),
                      _opt(TR, iters, **kw), str(tmp_path / "loop"), scale_bound=BOUND, seed=0, log=lambda *a: None,
                      views_per_step=4)
    with torch.no_grad():
        x, d, s, r = (t.detach() for t in out["model"].activated())
        vol = TR._query(x, d, s, r, case.center, case.nVoxel, case.sVoxel)
    psnr = S.psnr3d(case.vol_gt, vol.cpu())
    print("W = 4, 3D PSNR: initial %.3f, native %.3f (P %d), mini_trainer %.3f (P %d), difference %+.3f dB" % (
        ref["psnr"][0], psnr, out["P"], ref["psnr"][-1], ref["P"][-1], psnr - ref["psnr"][-1]))
    assert out["views_per_s"] == 4 * out["it_per_s"]
    assert psnr >= ref["psnr"][0] + 1.0
    assert abs(psnr - ref["psnr"][-1]) <= 0.2


def _blob(n, c0, sigma, rho):
    ax = -1 + (np.arange(n) + 0.5) * 2.0 / n
    X, Y, Z = np.meshgrid(ax, ax, ax, indexing="ij")
    return (rho * np.exp(-((X - c0[0]) ** 2 + (Y - c0[1]) ** 2 + (Z - c0[2]) ** 2) / (2 * sigma ** 2))).astype(np.float32)


def test_command_line(tmp_path, gpu):
    from r2_gaussian_amd import datagen as D
    from r2_gaussian_amd import scene as S
    n, iters = 64, 200
    vol = _blob(n, (0.1, -0.2, 0.05), 0.3, 0.6) + _blob(n, (-0.3, 0.25, -0.1), 0.12, 0.5) + _blob(n, (0.35, 0.3, 0.2), 0.08, 0.4)
    cfg = dict(S.CONE_BEAM, nVoxel=[n, n, n], nDetector=[128, 128], noise=False, totalAngle=360.0, startAngle=0.0)
    case = D.generate(vol, cfg, str(tmp_path / "data"), "phantom", n_train=50, n_test=20, seed=0)
    out = str(tmp_path / "out")
    common = ["--iterations", str(iters), "--densify_from_iter", "90", "--densify_until_iter", "150", "--position_lr_max_steps",
              str(iters), "--density_lr_max_steps", str(iters), "--scaling_lr_max_steps", str(iters), "--rotation_lr_max_steps",
              str(iters), "--test_iterations", "0", "100", "--checkpoint_iterations", "100"]
    r = subprocess.run([sys.executable, "-m", "r2_gaussian_amd.train", "-s", case, "-m", out, "--views_per_step", "4"] + common,
                       cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-5000:]
    # the layout tests/test_train_gpu.py::test_output_layout_and_keys checks
    pc = os.path.join(out, "point_cloud", "iteration_%d" % iters)
    for f in ("point_cloud.pickle", "vol_gt.npy", "vol_pred.npy"):
        assert os.path.exists(os.path.join(pc, f)), f
    assert np.load(os.path.join(pc, "vol_pred.npy")).shape == (64, 64, 64)
    assert os.path.exists(os.path.join(out, "ckpt", "chkpnt100.pth"))
    keys3d = ["psnr_3d", "ssim_3d", "ssim_3d_x", "ssim_3d_y", "ssim_3d_z"]
    keys2d = ["psnr_2d", "ssim_2d", "psnr_2d_projs", "ssim_2d_projs"]
    for it in (0, 1, 100, iters):
        d = os.path.join(out, "eval", "iter_%06d" % it)
        assert list(yaml.safe_load(open(os.path.join(d, "eval3d.yml")))) == keys3d
        for name, nv in (("render_train", 50), ("render_test", 20)):
            e = yaml.safe_load(open(os.path.join(d, "eval2d_%s.yml" % name)))
            assert list(e) == keys2d and len(e["psnr_2d_projs"]) == nv
    last = r.stdout.strip().splitlines()[-1]
    assert "it/s" in last and "views/s" in last, last
    e0 = yaml.safe_load(open(os.path.join(out, "eval", "iter_000000", "eval3d.yml")))
    e1 = yaml.safe_load(open(os.path.join(out, "eval", "iter_%06d" % iters, "eval3d.yml")))
    print("psnr_3d: iteration 0 %.3f, iteration %d %.3f; %s" % (e0["psnr_3d"], iters, e1["psnr_3d"], last))
    assert e1["psnr_3d"] > e0["psnr_3d"]
    r = subprocess.run([sys.executable, "-m", "r2_gaussian_amd.train", "-s", case, "-m", str(tmp_path / "no"), "--views_per_step",
                        "0"], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "usage:" in r.stderr and "--views_per_step" in r.stderr
    assert not os.path.exists(str(tmp_path / "no"))
