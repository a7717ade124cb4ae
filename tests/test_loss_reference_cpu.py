"""The float64 loss restatement (tests/loss_ref.py) that tests/test_losses_edges_gpu.py checks the fused kernels against,
pinned on the CPU: to tests/golden/train/losses.npz, which the reference's own loss_utils.py wrote (make_golden_train.py), and
to the float32 torch restatement in tests/mini_trainer.py.  Also the wrapper's argument checks, which run before any launch."""
import math
import os

import numpy as np
import pytest
import torch

from tests import loss_ref as R
from tests import mini_trainer as T

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "train", "losses.npz")


def _f32_l1_ssim(img, gt, w_l1, w_ssim):
    a = torch.from_numpy(np.asarray(img, np.float32)).reshape(1, *np.shape(img)[-2:]).requires_grad_(True)
    b = torch.from_numpy(np.asarray(gt, np.float32)).reshape(1, *np.shape(gt)[-2:])
    s = T.ssim(a, b)
    loss = w_l1 * (a - b).abs().mean() + w_ssim * (1.0 - s)
    loss.backward()
    return float(loss), float(s), a.grad[0].numpy().astype(np.float64)


@pytest.mark.parametrize("i", range(3))
def test_l1_ssim_restatement_matches_reference_fixture(i):
    """The reference's float32 values and autograd gradients lie within the derived float32 bounds of the float64
    restatement (their own rounding is float32 rounding of the same sums, in a different order)."""
    g = np.load(GOLDEN)
    img, gt = g["img%d" % i], g["gt%d" % i]
    ssim_part = R.l1_ssim64(img, gt, 0.0, 1.0)           # loss = 1 - SSIM: grad = -dSSIM/dimg
    b = R.l1_ssim_bounds(ssim_part)
    assert b["cond_ok"]
    assert abs(float(g["ssim_%d" % i]) - ssim_part["ssim"]) <= b["ssim"]
    np.testing.assert_array_less(np.abs(-g["ssim_grad%d" % i][0] - ssim_part["grad"]), b["grad"] + 1e-300)
    l1_part = R.l1_ssim64(img, gt, 1.0, 0.0)
    bl = R.l1_ssim_bounds(l1_part)
    assert abs(float(g["l1_%d" % i]) - l1_part["l1"]) <= bl["l1"]
    np.testing.assert_array_less(np.abs(g["l1_grad%d" % i][0] - l1_part["grad"]), bl["grad"] + 1e-300)
    # and the float32 reference agrees with the float64 restatement far inside the bound: the bound is not what pins it
    assert np.abs(-g["ssim_grad%d" % i][0] - ssim_part["grad"]).max() <= 1e-5 * np.abs(ssim_part["grad"]).max()


@pytest.mark.parametrize("i", range(2))
def test_tv_restatement_matches_reference_fixture(i):
    g = np.load(GOLDEN)
    vol = g["vol%d" % i]
    tv, grad, total, cnt = R.tv3d64(vol)
    b = R.tv3d_bounds(vol, total, cnt, grad)
    assert abs(float(g["tv_%d" % i]) - tv) <= b["tv"]
    assert abs(float(g["tv_sum_%d" % i]) - total) <= 1e-6 * total
    # torch adds the six +-1/cnt contributions in float: up to 6 roundings of terms of size 1/cnt (a zero may come out as
    # 1e-12), where the fused kernel divides an exact integer once
    np.testing.assert_allclose(g["tv_grad%d" % i], grad, rtol=0, atol=8 * R.U / cnt)


@pytest.mark.parametrize("hw,kind", [((1, 1), "rand"), ((1, 37), "rand"), ((37, 1), "rand"), ((5, 7), "rand"),
                                     ((33, 31), "rand"), ((40, 24), "equal"), ((24, 40), "zeros"), ((20, 30), "const"),
                                     ((48, 40), "blob"), ((30, 33), "large")])
def test_l1_ssim_restatement_matches_float32_torch(hw, kind):
    """Against mini_trainer's float32 conv2d evaluation, on the CPU: within the derived bounds, at shapes smaller than the
    window and with exact ties, zero images, constant images and a blob on a zero background."""
    rng = np.random.default_rng(hw[0] * 100 + hw[1])
    gt = rng.random(hw).astype(np.float32)
    img = np.clip(gt + 0.1 * rng.standard_normal(hw), 0, None).astype(np.float32)
    if kind == "equal":
        img = gt.copy()
    elif kind == "zeros":
        img, gt = np.zeros(hw, np.float32), np.zeros(hw, np.float32)
    elif kind == "const":
        img, gt = np.full(hw, 0.75, np.float32), np.full(hw, 0.5, np.float32)
    elif kind == "blob":
        yy, xx = np.mgrid[:hw[0], :hw[1]]
        gt = (2.0 * np.exp(-((yy - 20) ** 2 + (xx - 18) ** 2) / 60.0)).astype(np.float32)
        img = (gt * 1.05).astype(np.float32)
        img[:6, :6] = gt[:6, :6]
    elif kind == "large":
        gt, img = gt * 50, img * 50
    for w_l1, w_ssim in ((1.0, 0.25), (0.0, 1.0)):
        r = R.l1_ssim64(img, gt, w_l1, w_ssim)
        b = R.l1_ssim_bounds(r)
        assert b["cond_ok"]
        loss, s, grad = _f32_l1_ssim(img, gt, w_l1, w_ssim)
        assert abs(s - r["ssim"]) <= b["ssim"]
        assert abs(loss - r["loss"]) <= b["loss"]
        np.testing.assert_array_less(np.abs(grad - r["grad"]), b["grad"] + 1e-300)
    if kind == "zeros":
        assert r["ssim"] == 1.0 and not r["grad"].any()


def test_l1_ssim_restatement_is_the_autograd_derivative():
    """The analytic dL/dimg of the restatement equals float64 torch autograd through the same blur (no float32 anywhere)."""
    rng = np.random.default_rng(3)
    gt = rng.random((19, 23))
    img = np.clip(gt + 0.2 * rng.standard_normal(gt.shape), 0, None)
    img[:3, :3] = gt[:3, :3]
    w = torch.from_numpy(np.outer(R.window64(), R.window64())).view(1, 1, 11, 11)
    a = torch.from_numpy(img).view(1, 1, *img.shape).requires_grad_(True)
    b = torch.from_numpy(gt).view(1, 1, *gt.shape)
    conv = lambda t: torch.nn.functional.conv2d(t, w, padding=5)
    m1, m2 = conv(a), conv(b)
    s1, s2, s12 = conv(a * a) - m1 * m1, conv(b * b) - m2 * m2, conv(a * b) - m1 * m2
    S = ((2 * m1 * m2 + R.C1) * (2 * s12 + R.C2)) / ((m1 * m1 + m2 * m2 + R.C1) * (s1 + s2 + R.C2))
    loss = 0.7 * (a - b).abs().mean() + 0.4 * (1 - S.mean())
    loss.backward()
    r = R.l1_ssim64(img, gt, 0.7, 0.4)
    assert abs(float(loss) - r["loss"]) <= 1e-14
    np.testing.assert_allclose(r["grad"], a.grad[0, 0].numpy(), rtol=1e-10, atol=1e-16)


@pytest.mark.parametrize("shape", [(1, 1, 1), (1, 1, 4), (2, 1, 1), (1, 17, 33), (5, 7, 6)])
def test_tv_restatement_matches_torch(shape):
    """tv_3d_loss(vol, "mean") as the reference writes it, in float64 torch with autograd: value and gradient, including the
    1 x 1 x 1 volume without neighbour pairs (0 / 0: NaN, and a zero gradient)."""
    rng = np.random.default_rng(sum(shape))
    vol = np.floor(rng.random(shape) * 4)               # integer values: many exact zero differences
    v = torch.from_numpy(vol).requires_grad_(True)
    tv = T.tv3d_mean(v) if min(shape) > 0 and np.prod(shape) > 1 else None
    if tv is None:
        dx, dy, dz = (torch.diff(v, dim=k).abs().sum() for k in range(3))
        tv = (dx + dy + dz) / torch.tensor(0.0, dtype=torch.float64)
    tv.backward()
    ref, grad, _total, cnt = R.tv3d64(vol)
    if cnt == 0:
        assert math.isnan(ref) and math.isnan(float(tv))
        assert not grad.any() and not v.grad.numpy().any()
    else:
        assert abs(float(tv) - ref) <= 1e-15 * max(ref, 1.0)
        np.testing.assert_allclose(grad, v.grad.numpy(), rtol=1e-15, atol=0)


def test_float_fold_emulation():
    """The host emulation of the kernels' former float fold: exact where float32 is exact, and a float32 sum otherwise."""
    assert R.float_fold(np.ones(70000, np.float32)) == 70000.0
    p = np.random.default_rng(0).random(5000).astype(np.float32)
    assert abs(float(R.float_fold(p)) - p.astype(np.float64).sum()) <= 5000 * 20 * R.U


@pytest.mark.parametrize("img,gt", [((1, 8, 9), (1, 8, 10)), ((1, 8, 9), (1, 9, 9)), ((8, 9), (1, 16, 18)),
                                    ((1, 16, 18), (8, 9)), ((2, 8, 9), (2, 8, 9)), ((8, 9), (3, 8, 9)), ((1, 1, 8, 9), (8, 9))])
def test_image_loss_rejects_mismatched_shapes(img, gt):
    """gt must be the image's size, and both one [H, W] or [1, H, W] projection: checked before the GPU is touched."""
    from r2_gaussian_amd.losses import image_loss
    with pytest.raises(ValueError):
        image_loss(torch.zeros(img), torch.zeros(gt))
