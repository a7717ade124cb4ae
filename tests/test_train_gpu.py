"""GPU: the native trainer (python -m r2_gaussian_amd.train) end to end on a case written by datagen -- output layout, the
model file, a PSNR gain, resuming from a checkpoint -- and its loop against tests/mini_trainer.py (torch Adam) on the same
in-memory case."""
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
ITERS = 1000


def _blob(n, c0, sigma, rho):
    ax = -1 + (np.arange(n) + 0.5) * 2.0 / n
    X, Y, Z = np.meshgrid(ax, ax, ax, indexing="ij")
    return (rho * np.exp(-((X - c0[0]) ** 2 + (Y - c0[1]) ** 2 + (Z - c0[2]) ** 2) / (2 * sigma ** 2))).astype(np.float32)


@pytest.fixture(scope="module")
def trained(tmp_path_factory):
    """A seeded 64^3 phantom (128^2 detector, 50 train / 20 test views), trained for ITERS iterations with one
    densification (iteration 500) and a checkpoint there."""
    from r2_gaussian_amd import datagen as D
    from r2_gaussian_amd import scene as S
    base = tmp_path_factory.mktemp("train")
    n = 64
    vol = _blob(n, (0.1, -0.2, 0.05), 0.3, 0.6) + _blob(n, (-0.3, 0.25, -0.1), 0.12, 0.5) + _blob(n, (0.35, 0.3, 0.2), 0.08, 0.4)
    cfg = dict(S.CONE_BEAM, nVoxel=[n, n, n], nDetector=[128, 128], noise=False, totalAngle=360.0, startAngle=0.0)
    case = D.generate(vol, cfg, str(base / "data"), "phantom", n_train=50, n_test=20, seed=0)
    out = str(base / "out")
    common = ["--iterations", str(ITERS), "--densify_from_iter", "450", "--densify_until_iter", "550",
              "--position_lr_max_steps", str(ITERS), "--density_lr_max_steps", str(ITERS), "--scaling_lr_max_steps",
              str(ITERS), "--rotation_lr_max_steps", str(ITERS), "--test_iterations", "0", "500", "--quiet"]
    r = subprocess.run([sys.executable, "-m", "r2_gaussian_amd.train", "-s", case, "-m", out, "--checkpoint_iterations", "500"]
                       + common, cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-5000:]
    return dict(case=case, out=out, common=common, stdout=r.stdout, base=base)


def test_output_layout_and_keys(trained):
    out = trained["out"]
    pc = os.path.join(out, "point_cloud", "iteration_%d" % ITERS)
    for f in ("point_cloud.pickle", "vol_gt.npy", "vol_pred.npy"):
        assert os.path.exists(os.path.join(pc, f)), f
    assert np.load(os.path.join(pc, "vol_pred.npy")).shape == (64, 64, 64)
    assert os.path.exists(os.path.join(out, "ckpt", "chkpnt500.pth"))
    keys3d = ["psnr_3d", "ssim_3d", "ssim_3d_x", "ssim_3d_y", "ssim_3d_z"]
    keys2d = ["psnr_2d", "ssim_2d", "psnr_2d_projs", "ssim_2d_projs"]
    for it in (0, 1, 500, ITERS):
        d = os.path.join(out, "eval", "iter_%06d" % it)
        assert list(yaml.safe_load(open(os.path.join(d, "eval3d.yml")))) == keys3d
        for name, nv in (("render_train", 50), ("render_test", 20)):
            e = yaml.safe_load(open(os.path.join(d, "eval2d_%s.yml" % name)))
            assert list(e) == keys2d and len(e["psnr_2d_projs"]) == nv
    assert "it/s" in trained["stdout"].strip().splitlines()[-1]


def test_model_file_loads_and_psnr_gains(trained):
    from r2_gaussian_amd import model_io
    out = trained["out"]
    m = model_io.load_point_cloud(os.path.join(out, "point_cloud", "iteration_%d" % ITERS, "point_cloud.pickle"))
    P = m["xyz"].shape[0]
    assert P > 0 and m["density"].shape == (P, 1) and m["scaling"].shape == (P, 3) and m["rotation"].shape == (P, 4)
    assert m["scale_bound"] is not None
    e0 = yaml.safe_load(open(os.path.join(out, "eval", "iter_000000", "eval3d.yml")))
    e1 = yaml.safe_load(open(os.path.join(out, "eval", "iter_%06d" % ITERS, "eval3d.yml")))
    print("psnr_3d: iteration 0 %.3f, iteration %d %.3f" % (e0["psnr_3d"], ITERS, e1["psnr_3d"]))
    assert e1["psnr_3d"] >= e0["psnr_3d"] + 2.0
    # the saved volume is the evaluated one
    from r2_gaussian_amd.metrics import metric_vol
    pc = os.path.join(out, "point_cloud", "iteration_%d" % ITERS)
    psnr, _ = metric_vol(np.load(os.path.join(pc, "vol_gt.npy")), np.load(os.path.join(pc, "vol_pred.npy")))
    assert abs(psnr - e1["psnr_3d"]) < 1e-3


def test_resume_from_checkpoint(trained):
    out2 = str(trained["base"] / "resumed")
    ck = os.path.join(trained["out"], "ckpt", "chkpnt500.pth")
    r = subprocess.run([sys.executable, "-m", "r2_gaussian_amd.train", "-s", trained["case"], "-m", out2, "--start_checkpoint", ck]
                       + trained["common"], cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-5000:]
    assert os.path.exists(os.path.join(out2, "point_cloud", "iteration_%d" % ITERS, "point_cloud.pickle"))
    e = yaml.safe_load(open(os.path.join(out2, "eval", "iter_%06d" % ITERS, "eval3d.yml")))
    e0 = yaml.safe_load(open(os.path.join(trained["out"], "eval", "iter_000000", "eval3d.yml")))
    assert e["psnr_3d"] >= e0["psnr_3d"] + 2.0
    assert not os.path.exists(os.path.join(out2, "eval", "iter_000001"))   # iterations before the checkpoint are not rerun


def test_unknown_flag_is_an_error():
    r = subprocess.run([sys.executable, "-m", "r2_gaussian_amd.train", "-s", "x", "--no_such_flag", "1"], cwd=ROOT,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "unrecognized arguments" in r.stderr


def test_loop_matches_mini_trainer(tmp_path):
    """The loop on a mini_trainer.Case ends within 0.2 dB of 3D PSNR of mini_trainer.train (torch Adam) with the same options
    and seed: both draw the same view order, TV centres and split samples."""
    from r2_gaussian_amd import train as TR
    from r2_gaussian_amd import scene as S
    iters = 600
    kw = dict(iterations=iters, densify_from_iter=150, densify_until_iter=500, densification_interval=100)
    case = T.Case(detector=128, n_vol=64, n_views=30, p_gt=8000, n_init=3000, seed=2)
    ref = T.train(case, T.Opt(**kw), "hip", eval_every=iters, seed=0, fused_losses=True, fused_densify=True)
    opt = TR.OptimizationParams(**kw, position_lr_max_steps=iters, density_lr_max_steps=iters, scaling_lr_max_steps=iters,
                                rotation_lr_max_steps=iters)
    geo = dict(nVoxel=list(case.nVoxel), sVoxel=list(case.sVoxel), offOrigin=list(case.center), dVoxel=case.dVoxel.tolist())
    init = np.concatenate([case.init_xyz.numpy(), case.init_density.numpy()[:, None]], 1)
    out = TR.training(case.views, [p.numpy() for p in case.projs], [], [], case.vol_gt.numpy(), geo, init, opt,
                      str(tmp_path / "loop"), scale_bound=(T.Opt.scale_min * 2.0, T.Opt.scale_max * 2.0), seed=0,
                      log=lambda *a: None)
    with torch.no_grad():
        x, d, s, r = (t.detach() for t in out["model"].activated())
        vol = TR._query(x, d, s, r, case.center, case.nVoxel, case.sVoxel)
    psnr = S.psnr3d(case.vol_gt, vol.cpu())
    print("3D PSNR: native %.3f (P %d), mini_trainer %.3f (P %d)" % (psnr, out["P"], ref["psnr"][-1], ref["P"][-1]))
    assert psnr > ref["psnr"][0] + 1.0
    assert abs(psnr - ref["psnr"][-1]) <= 0.2
