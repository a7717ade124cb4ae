"""tests/golden/metrics/: values written by the REFERENCE's own Python -- metric_vol and metric_proj of
r2_gaussian/utils/image_utils.py:90-184 and the per-slice ssim / psnr they call (utils/loss_utils.py:57-104, image_utils.py:67-87),
evaluated on the CPU -- so that r2_gaussian_amd/metrics.py is pinned against them (tests/test_metrics_gpu.py).  Needs
/root/reference; image_utils imports nothing that needs a GPU or a stub.

    python tests/golden/make_golden_metrics.py

Volume cases (vol_*.npz): gt, pred, psnr (pixel_max 1), psnr_none (pixel_max None), ssim, ssim_axes and the per-slice SSIM of
every axis (ssim_slices_0/1/2, 0 where the ground-truth slice is all <= 0: the values metric_vol sums).  Projection cases
(proj_*.npz): the [N, H, W] image stacks (the test rebuilds the [H, W, N] view train.py passes), axis, and for psnr and ssim
the mean and the per-slice list metric_proj returns.
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
OUT = os.path.join(HERE, "metrics")


def smooth_field(shape, g, passes=2):
    """Structured values in [0, 1]: uniform noise box-blurred along every axis (SSIM on pure noise says little)."""
    a = torch.rand(*shape, generator=g, dtype=torch.float64)
    for _ in range(passes):
        for ax in range(len(shape)):
            a = (a + a.roll(1, ax) + a.roll(-1, ax)) / 3.0
    a = (a - a.min()) / (a.max() - a.min() + 1e-12)
    return a.float()


def noisy(a, g, sigma):
    return (a + sigma * torch.randn(a.shape, generator=g)).clamp_min(0.0)


def per_slice_ssim(ssim, a, b, axis):
    out = []
    for i in range(a.shape[axis]):
        s1, s2 = a.select(axis, i), b.select(axis, i)
        out.append(float(ssim(s1[None, None], s2[None, None])) if s1.max() > 0 else 0.0)
    return np.array(out, np.float32)


def vol_case(name, a, b, metric_vol, ssim):
    s, axes = metric_vol(a, b, "ssim")
    p, _ = metric_vol(a, b, "psnr")
    pn, _ = metric_vol(a, b, "psnr", pixel_max=None)
    np.savez_compressed(os.path.join(OUT, name + ".npz"), gt=a.numpy(), pred=b.numpy(), psnr=np.float64(p),
                        psnr_none=np.float64(pn), ssim=np.float64(s), ssim_axes=np.array(axes, np.float64),
                        **{"ssim_slices_%d" % ax: per_slice_ssim(ssim, a, b, ax) for ax in range(3)})
    print(name, tuple(a.shape), "psnr %.4f / %.4f  ssim %.6f" % (p, pn, s), ["%.6f" % x for x in axes])


def proj_case(name, gt_images, images, axis, metric_proj):
    """gt_images / images: lists of [1, H, W] projections, stacked as train.py:281-284 does."""
    gts = torch.concat(gt_images, 0)
    prs = torch.concat(images, 0)
    view = (lambda t: t.permute(1, 2, 0)) if axis == 2 else (lambda t: t)
    out = {}
    for m in ("psnr", "ssim"):
        mean, per = metric_proj(view(gts), view(prs), m, axis=axis)
        out[m] = np.float64(mean)
        out[m + "_slices"] = np.array(per, np.float32)
    np.savez_compressed(os.path.join(OUT, name + ".npz"), gt=gts.numpy(), pred=prs.numpy(), axis=np.int64(axis), **out)
    print(name, tuple(gts.shape), "axis", axis, "psnr %.4f  ssim %.6f" % (out["psnr"], out["ssim"]))


if __name__ == "__main__":
    os.makedirs(OUT, exist_ok=True)
    sys.path.insert(0, REF)
    from r2_gaussian.utils.image_utils import metric_proj, metric_vol
    from r2_gaussian.utils.loss_utils import ssim
    g = torch.Generator().manual_seed(2024)

    # non-cubic volumes, an all-zero ground-truth slice on each axis
    a = smooth_field((37, 29, 53), g)
    a[5], a[:, 7], a[:, :, 11] = 0.0, 0.0, 0.0
    vol_case("vol_37x29x53", a, noisy(a, g, 0.04), metric_vol, ssim)
    a = smooth_field((12, 10, 14), g, passes=1)
    a[3], a[:, 0], a[:, :, 13] = 0.0, 0.0, 0.0
    vol_case("vol_12x10x14", a, noisy(a, g, 0.08), metric_vol, ssim)
    # slices smaller than the 11 x 11 window
    a = smooth_field((5, 7, 6), g, passes=1)
    vol_case("vol_5x7x6", a, noisy(a, g, 0.05), metric_vol, ssim)
    # a dimension of 1
    a = smooth_field((1, 9, 13), g, passes=1)
    vol_case("vol_1x9x13", a, noisy(a, g, 0.05), metric_vol, ssim)
    # exact match: PSNR inf, SSIM 1
    a = smooth_field((8, 9, 10), g, passes=1)
    vol_case("vol_exact_8x9x10", a, a.clone(), metric_vol, ssim)
    # no slice counts: SSIM NaN on every axis (sum / 0)
    vol_case("vol_zero_gt_4x5x6", torch.zeros(4, 5, 6), smooth_field((4, 5, 6), g, passes=1), metric_vol, ssim)

    # projections, stacked as train.py builds them: [1, H, W] images -> concat -> permute(1, 2, 0), axis 2
    H, W, N = 33, 40, 6
    gt_images = [smooth_field((1, H, W), g) * (0.5 + i / N) for i in range(N)]
    images = [noisy(x, g, 0.03) for x in gt_images]
    gt_images[2] = torch.zeros(1, H, W)            # left out of the count
    images[4] = gt_images[4].clone()               # exact match: PSNR inf, SSIM 1
    proj_case("proj_stack_33x40x6", gt_images, images, 2, metric_proj)
    H, W, N = 20, 24, 4
    gt_images = [smooth_field((1, H, W), g) for _ in range(N)]
    images = [noisy(x, g, 0.05) for x in gt_images]
    images[1] = torch.zeros(1, H, W)               # prediction max 0: NaN, propagates to the mean
    proj_case("proj_nan_20x24x4", gt_images, images, 2, metric_proj)
    gt_images = [smooth_field((1, 5, 7), g, passes=1) for _ in range(3)]
    images = [noisy(x, g, 0.05) for x in gt_images]
    proj_case("proj_axis0_3x5x7", gt_images, images, 0, metric_proj)
    print("wrote", sorted(os.listdir(OUT)))
