"""Evaluation of a reconstruction on the MI355X kernels (csrc/metric_ops.hip): drop-in replacements for ``metric_vol`` and
``metric_proj`` of r2_gaussian/utils/image_utils.py:90-184 (train.py:241-355, test.py:114-131) with the reference's argument
order (``img1`` is the ground truth), return types and odd cases:

* a slice whose ground-truth maximum is <= 0 contributes 0 and is left out of the count; the mean is sum / count, NaN when no
  slice counts;
* ``metric_proj`` divides every slice of both inputs by its own maximum: a prediction slice with maximum 0 gives NaN, which
  propagates to the mean; a slice with zero error has PSNR inf;
* ``metric_vol(..., pixel_max=None)`` takes the ground truth's maximum.

Each call makes ONE host synchronisation (the per-slice table is read back once, the means are finished from it on the host
in a fixed order).  CUDA tensors are used in place; numpy arrays and CPU tensors are copied to the GPU once; there is no CPU
compute path.  ``slice_metrics`` returns the per-slice table on the device, for loggers that must not synchronise.
"""
import math

import numpy as np
import torch

from . import _lib
from ._boundary import _F32, call


def _to_device(t, device=None):
    if isinstance(t, torch.Tensor):
        if t.is_cuda:
            return t if t.dtype == _F32 else t.to(_F32)
        return t.to(device=device or torch.device("cuda", torch.cuda.current_device()), dtype=_F32)
    a = np.asarray(t)
    if any(s < 0 for s in a.strides):
        a = np.ascontiguousarray(a)
    return torch.from_numpy(a).to(device=device or torch.device("cuda", torch.cuda.current_device()), dtype=_F32)


def _storage_order(t):
    """-> perm such that t.permute(perm) is C-contiguous, or None (size-1 axes may go anywhere)."""
    perm = sorted(range(t.dim()), key=lambda d: (-t.stride(d), d))
    return perm if t.permute(perm).is_contiguous() else None


def _inputs(img1, img2):
    """-> (gt, pred, perm): both on the same GPU, float32, gt.permute(perm) and pred.permute(perm) C-contiguous.  A strided view
    whose storage is C-contiguous in some axis order passes that storage without a copy; anything else is made contiguous."""
    gt = _to_device(img1)
    pred = _to_device(img2, gt.device)
    if gt.dim() != 3 or gt.shape != pred.shape:
        raise ValueError("expected two 3D arrays of the same shape, got %s and %s" % (tuple(gt.shape), tuple(pred.shape)))
    if pred.device != gt.device:
        pred = pred.to(gt.device)
    perm = _storage_order(gt) or _storage_order(pred) or [0, 1, 2]
    return gt, pred, perm


def _run(gt, pred, perm, axes, flags, out):
    """r2_metric_slices for every view axis in `axes`, written one after the other into out [sum of slice counts, 4]."""
    g = gt.permute(perm)
    p = pred.permute(perm)
    g = g if g.is_contiguous() else g.contiguous()
    p = p if p.is_contiguous() else p.contiguous()
    n = [int(s) for s in g.shape]
    L = _lib.lib()
    saxes = [perm.index(a) for a in axes]
    scratch = torch.empty(max(L.r2_metric_slices_scratch_floats(*n, a) for a in saxes), dtype=_F32, device=g.device)
    row = 0
    for a in saxes:
        call("r2_metric_slices", g.device, *n, a, g, p, flags, out[row:], scratch)
        row += n[a]
    return out


@torch.no_grad()
def slice_metrics(gt, pred, axis, normalize=False):
    """-> device tensor [n, 4] of the slices along `axis`: {mean SSIM, sum (gt - pred)^2, max gt, max pred}; with `normalize`
    both are divided by each slice's own maximum first (metric_proj), the maxima stay those of the inputs.  No host sync."""
    g, p, perm = _inputs(gt, pred)
    out = torch.empty(g.shape[axis], 4, dtype=_F32, device=g.device)
    return _run(g, p, perm, [axis], _lib.R2_METRIC_SSIM | (_lib.R2_METRIC_NORMALIZE if normalize else 0), out)


def _host_slices(img1, img2, axes, flags):
    """-> ([per-slice numpy table [n_axis, 4] per axis], slice area per axis, voxel count): one synchronisation.
    axes None: the one axis whose slices are contiguous in memory (for sums over the whole array)."""
    g, p, perm = _inputs(img1, img2)
    axes = [perm[0]] if axes is None else axes
    counts = [int(g.shape[a]) for a in axes]
    out = torch.empty(sum(counts), 4, dtype=_F32, device=g.device)
    host = _run(g, p, perm, axes, flags, out).cpu().numpy().astype(np.float64)
    tabs = np.split(host, np.cumsum(counts)[:-1])
    return tabs, [g.numel() // c for c in counts], g.numel()


def _masked_mean(values, gt_max):
    """The reference's sum / count over the slices whose ground truth has a positive maximum (others contribute 0)."""
    valid = gt_max > 0
    per = np.where(valid, values, 0.0).astype(np.float32)
    count = int(valid.sum())
    total = float(per.astype(np.float64).sum())
    return (total / count if count else math.nan), per.tolist()


def _psnr(pixel_max, sse, n):
    with np.errstate(divide="ignore", invalid="ignore"):
        return 10.0 * np.log10(np.float64(pixel_max) ** 2 / (np.asarray(sse, np.float64) / n))


def _vol_psnr(tab, n, pixel_max):
    """3D PSNR from the per-slice SSE / maxima of any one axis, summed in slice order."""
    pm = float(tab[:, 2].max()) if pixel_max is None else pixel_max
    return float(_psnr(pm, tab[:, 1].sum(), n))


def _vol_ssim(tabs):
    per_axis = [_masked_mean(t[:, 0], t[:, 2])[0] for t in tabs]
    return float(np.mean(per_axis)), per_axis


@torch.no_grad()
def metric_vol(img1, img2, metric="psnr", pixel_max=1.0):
    """metric_vol of image_utils.py:90-132.  psnr -> (float, None): 10 log10(pixel_max^2 / mean (img1 - img2)^2), pixel_max None =
    max img1.  ssim -> (float, [3 floats]): per axis the mean 2D SSIM of the slices whose ground truth is not all <= 0, and
    the mean of the three."""
    assert metric in ("psnr", "ssim")
    if metric == "psnr":
        (tab,), _, n = _host_slices(img1, img2, None, 0)
        return _vol_psnr(tab, n, pixel_max), None
    tabs, _, _ = _host_slices(img1, img2, [0, 1, 2], _lib.R2_METRIC_SSIM)
    return _vol_ssim(tabs)


@torch.no_grad()
def metric_vol_both(img1, img2, pixel_max=1.0):
    """-> (psnr, ssim, [3 ssim per axis]) of metric_vol from ONE pass over the three axes and one synchronisation."""
    tabs, _, n = _host_slices(img1, img2, [0, 1, 2], _lib.R2_METRIC_SSIM)
    ssim, per_axis = _vol_ssim(tabs)
    return _vol_psnr(tabs[0], n, pixel_max), ssim, per_axis


@torch.no_grad()
def metric_proj(img1, img2, metric="psnr", axis=2, pixel_max=1.0):
    """metric_proj of image_utils.py:135-184: every slice along `axis` (a projection of the [H, W, N] stack train.py builds)
    divided by its own maximum, then per-slice PSNR (against pixel_max) or SSIM.  -> (mean, [per-slice floats])."""
    assert axis in (0, 1, 2)
    assert metric in ("psnr", "ssim")
    flags = _lib.R2_METRIC_NORMALIZE | (_lib.R2_METRIC_SSIM if metric == "ssim" else 0)
    (tab,), (area,), _ = _host_slices(img1, img2, [axis], flags)
    values = tab[:, 0] if metric == "ssim" else _psnr(pixel_max, tab[:, 1], area)
    return _masked_mean(values, tab[:, 2])
