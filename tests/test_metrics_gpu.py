"""The evaluation metrics on the device (csrc/metric_ops.hip, r2_gaussian_amd/metrics.py) against values written by the
reference's own metric_vol / metric_proj (tests/golden/metrics/, tests/golden/make_golden_metrics.py; tests/golden/model_io/),
against a float64 restatement of the per-slice SSIM on a voxelized volume, and for determinism and layout independence."""
import glob
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
VOLS = sorted(glob.glob(os.path.join(GOLD, "metrics", "vol_*.npz")))
PROJS = sorted(glob.glob(os.path.join(GOLD, "metrics", "proj_*.npz")))
SSIM_TOL, MEAN_TOL, PSNR_TOL = 5e-6, 1e-5, 1e-4


def close(got, want, tol, what):
    """|got - want| <= tol elementwise, with NaN and +-inf exactly where the reference has them."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, what
    assert np.array_equal(np.isnan(got), np.isnan(want)), (what, got, want)
    inf = np.isinf(want)
    assert np.array_equal(np.isinf(got), inf) and np.array_equal(got[inf], want[inf]), (what, got, want)
    fin = np.isfinite(want)
    err = np.abs(got[fin] - want[fin])
    assert err.size == 0 or err.max() <= tol, (what, err.max())


def name(p):
    return os.path.splitext(os.path.basename(p))[0]


@pytest.mark.parametrize("path", VOLS, ids=[name(p) for p in VOLS])
def test_metric_vol_matches_the_reference(path, gpu):
    from r2_gaussian_amd import metrics as Mx
    z = np.load(path)
    gt, pred = torch.from_numpy(z["gt"]).to(gpu), torch.from_numpy(z["pred"]).to(gpu)
    p, none = Mx.metric_vol(gt, pred, "psnr")
    assert none is None and isinstance(p, float)
    close(p, z["psnr"], PSNR_TOL, "psnr")
    close(Mx.metric_vol(gt, pred, "psnr", pixel_max=None)[0], z["psnr_none"], PSNR_TOL, "psnr, pixel_max None")
    s, axes = Mx.metric_vol(gt, pred, "ssim")
    assert isinstance(s, float) and isinstance(axes, list) and len(axes) == 3
    close(s, z["ssim"], MEAN_TOL, "ssim")
    close(axes, z["ssim_axes"], MEAN_TOL, "ssim per axis")
    for ax in range(3):
        t = Mx.slice_metrics(gt, pred, ax).cpu().numpy()
        assert t.shape == (gt.shape[ax], 4)
        counted = t[:, 2] > 0
        close(np.where(counted, t[:, 0], 0.0), z["ssim_slices_%d" % ax], SSIM_TOL, "ssim slices of axis %d" % ax)
        np.testing.assert_array_equal(t[:, 2], z["gt"].max(axis=tuple(d for d in range(3) if d != ax)))
        np.testing.assert_array_equal(t[:, 3], z["pred"].max(axis=tuple(d for d in range(3) if d != ax)))
    # numpy arrays and CPU tensors are copied to the GPU, and give what the device tensors give
    for a, b in ((z["gt"], z["pred"]), (gt.cpu(), pred.cpu())):
        s2, axes2 = Mx.metric_vol(a, b, "ssim")
        np.testing.assert_array_equal([s2] + axes2, [s] + axes)


@pytest.mark.parametrize("path", PROJS, ids=[name(p) for p in PROJS])
def test_metric_proj_matches_the_reference(path, gpu):
    from r2_gaussian_amd import metrics as Mx
    z = np.load(path)
    axis = int(z["axis"])
    gts, prs = torch.from_numpy(z["gt"]).to(gpu), torch.from_numpy(z["pred"]).to(gpu)
    view = (lambda t: t.permute(1, 2, 0)) if axis == 2 else (lambda t: t)   # train.py:281-284
    for m, tol in (("psnr", PSNR_TOL), ("ssim", SSIM_TOL)):
        mean, per = Mx.metric_proj(view(gts), view(prs), m, axis=axis)
        assert isinstance(mean, float) and isinstance(per, list) and len(per) == gts.shape[0]
        close(mean, z[m], max(tol, MEAN_TOL), m + " mean")
        close(per, z[m + "_slices"], tol, m + " per slice")


def test_model_io_fixture_at_the_same_bounds(gpu):
    from r2_gaussian_amd import metrics as Mx
    z = np.load(os.path.join(GOLD, "model_io", "metrics.npz"))
    s, axes = Mx.metric_vol(z["vol_gt"], z["vol_pred"], "ssim")
    close(s, z["ssim"], MEAN_TOL, "ssim")
    close(axes, z["ssim_axes"], MEAN_TOL, "ssim per axis")
    close(Mx.metric_vol(z["vol_gt"], z["vol_pred"], "psnr")[0], z["psnr"], PSNR_TOL, "psnr")


def ssim_slices_f64(a, b, axis):
    """Per-slice mean SSIM of every slice along `axis`, batched, float64, separable window, zero padding (loss_utils.py:57-104)."""
    x = a.double().movedim(axis, 0)[:, None]
    y = b.double().movedim(axis, 0)[:, None]
    g = torch.exp(-((torch.arange(11, dtype=torch.float64) - 5) ** 2) / (2 * 1.5 ** 2))
    g = g / g.sum()
    blur = lambda t: F.conv2d(F.conv2d(t, g.view(1, 1, 11, 1), padding=(5, 0)), g.view(1, 1, 1, 11), padding=(0, 5))
    m1, m2 = blur(x), blur(y)
    s1, s2, s12 = blur(x * x) - m1 * m1, blur(y * y) - m2 * m2, blur(x * y) - m1 * m2
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    S = (2 * m1 * m2 + C1) * (2 * s12 + C2) / ((m1 * m1 + m2 * m2 + C1) * (s1 + s2 + C2))
    return S.mean(dim=(1, 2, 3))


@pytest.fixture(scope="module")
def voxelized(gpu):
    """A seeded cloud voxelized on a 96 x 128 x 80 grid, and a noisy prediction of it."""
    from r2_gaussian_amd import GaussianVoxelizationSettings, GaussianVoxelizer
    from r2_gaussian_amd import scene as S
    c = S.make_cloud(3000, seed=21)
    st = GaussianVoxelizationSettings(1.0, 96, 128, 80, 2.0, 2.0, 2.0, 0.0, 0.0, 0.0, False, False)
    vol, _ = GaussianVoxelizer(st)(means3D=c.xyz.to(gpu), opacities=c.density.to(gpu), scales=c.scales.to(gpu),
                                   rotations=c.rotations.to(gpu))
    g = torch.Generator().manual_seed(3)
    gt = vol.detach()
    pred = (gt + 0.05 * float(gt.max()) * torch.randn(gt.shape, generator=g).to(gpu)).clamp_min(0.0)
    return gt, pred


def test_every_slice_against_a_float64_restatement(voxelized):
    from r2_gaussian_amd import metrics as Mx
    gt, pred = voxelized
    assert float(gt.max()) > 0.1
    for ax in range(3):
        got = Mx.slice_metrics(gt, pred, ax).cpu().double()
        want = ssim_slices_f64(gt.cpu(), pred.cpu(), ax)
        err = (got[:, 0] - want).abs().max().item()
        assert err <= SSIM_TOL, (ax, err)
        sse = ((gt.cpu().double() - pred.cpu().double()) ** 2).movedim(ax, 0).sum(dim=(1, 2))
        assert torch.allclose(got[:, 1], sse, rtol=1e-5, atol=1e-6), ax


def test_bit_reproducible_and_layout_independent(voxelized, gpu):
    from r2_gaussian_amd import metrics as Mx
    gt, pred = voxelized
    for ax in range(3):
        for norm in (False, True):
            a = Mx.slice_metrics(gt, pred, ax, normalize=norm)
            b = Mx.slice_metrics(gt, pred, ax, normalize=norm)
            assert torch.equal(a.nan_to_num(7.0), b.nan_to_num(7.0)), (ax, norm)
    assert Mx.metric_vol(gt, pred, "ssim") == Mx.metric_vol(gt, pred, "ssim")
    # an [H, W, N] view of [N, H, W] storage (train.py's stack) gives exactly what its contiguous copy gives
    g = torch.Generator().manual_seed(9)
    st_gt = torch.rand(12, 70, 90, generator=g).to(gpu)
    st_pr = (st_gt + 0.05 * torch.randn(12, 70, 90, generator=g).to(gpu)).clamp_min(0.0)
    vg, vp = st_gt.permute(1, 2, 0), st_pr.permute(1, 2, 0)
    for m in ("psnr", "ssim"):
        assert Mx.metric_proj(vg, vp, m) == Mx.metric_proj(vg.contiguous(), vp.contiguous(), m), m
    t_view = Mx.slice_metrics(vg, vp, 2, normalize=True)
    assert torch.equal(t_view, Mx.slice_metrics(vg.contiguous(), vp.contiguous(), 2, normalize=True))
    # slice_metrics agrees with metric_proj
    _, per = Mx.metric_proj(vg, vp, "ssim")
    assert per == t_view[:, 0].cpu().tolist()
    # a view that no permutation makes contiguous is copied: same values as the copy
    sub_g, sub_p = st_gt[:, ::2], st_pr[:, ::2]
    assert Mx.metric_vol(sub_g, sub_p, "ssim") == Mx.metric_vol(sub_g.contiguous(), sub_p.contiguous(), "ssim")
    # other dtypes are converted to float32
    assert Mx.metric_vol(gt.double(), pred.double(), "psnr") == Mx.metric_vol(gt, pred, "psnr")


def test_evaluate_volume_on_the_device(gpu):
    from r2_gaussian_amd import model_io as M
    model = M.load_point_cloud(os.path.join(GOLD, "model_io", "point_cloud.pickle"), device=gpu)
    cfg = {"nVoxel": [40, 36, 28], "sVoxel": [6.0, 6.0, 6.0], "offOrigin": [0.0, 0.0, 0.0]}
    vol = M.evaluate_volume(model, cfg)["vol"]
    g = torch.Generator().manual_seed(4)
    vol_gt = (vol + 0.02 * float(vol.max()) * torch.randn(vol.shape, generator=g).to(gpu)).clamp_min(0.0)
    host = M.evaluate_volume(model, cfg, vol_gt=vol_gt)
    dev = M.evaluate_volume(model, cfg, vol_gt=vol_gt, metrics="device")
    assert sorted(host) == sorted(dev)
    assert torch.equal(host["vol"], dev["vol"])
    close(dev["psnr_3d"], host["psnr_3d"], PSNR_TOL, "psnr_3d")
    for k in ("ssim_3d", "ssim_3d_x", "ssim_3d_y", "ssim_3d_z"):
        close(dev[k], host[k], MEAN_TOL, k)
