"""Conditioning of measured projections on the MI355X (csrc/projections.hip, csrc/destripe.hip; include/r2hip.h:
r2_proj_resize, r2_proj_median, r2_proj_destripe_sort, r2_proj_destripe_mean): what the reference's real-data converter does to
a measured stack with cv2 and numpy -- lower clamp, row shift, ``cv2.resize``, crop -- as one fused pass, a median filter
against the isolated outliers of measured data (zingers, hot pixels, NaN read-outs), which ``weights.fill_unmeasured`` only
handles once they are known, and stripe removal against the defect that no single projection shows: a detector pixel that is
slightly off in every view, a ring in the reconstruction.  ``prepare_real.py`` is the command line on top of these.

Projections are [H,W] or [V,H,W] tensors on the GPU and so are the results: a host array raises, there is no CPU fallback.
Inputs of another dtype or layout are converted to contiguous float32 first.  No host synchronisation.
"""
import math
import operator

import torch

from . import _lib
from ._boundary import call, f32c, require_gpu, workspace

_F32 = torch.float32
INTERPOLATIONS = {"linear": 0, "area": 1}
DESTRIPE_METHODS = {"sort": 0, "mean": 1}


def destripe_max_views():
    """R2_DESTRIPE_MAX_VIEWS of the loaded library: the views that method="sort" orders in the LDS."""
    return int(_lib.lib().r2_proj_destripe_max_views())


def _stack(projs, name="projs"):
    """-> (contiguous float32 [V,H,W], whether the caller gave [H,W])."""
    if not isinstance(projs, torch.Tensor):
        raise _lib.R2HipError("%s must be a GPU tensor: the MI355X kernels have no CPU fallback" % name)
    require_gpu(projs, name)
    if projs.dim() not in (2, 3) or projs.shape[-1] < 1 or projs.shape[-2] < 1:
        raise ValueError("%s must be [H,W] or [V,H,W] with H, W >= 1, got shape %s" % (name, tuple(projs.shape)))
    p = f32c(projs.detach() if projs.requires_grad else projs)
    if p.shape[-2] * p.shape[-1] >= 2 ** 31 or p.numel() >= 2 ** 38:
        raise ValueError("%s of shape %s is too large for one call: process it in batches of views" % (name, tuple(projs.shape)))
    return (p[None] if p.dim() == 2 else p), p.dim() == 2


def _pair(value, name, lowest=None):
    try:
        a, b = value
        ok = int(a) == a and int(b) == b and (lowest is None or min(a, b) >= lowest)
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError("%s must be two integers%s, got %r" % (name, "" if lowest is None else " >= %d" % lowest, value))
    return int(a), int(b)


def resize(projs, size, interpolation="linear", shift=(0, 0), lo=None, crop=None, out=None):
    """Shift, lower clamp, resize, crop, in this order and in one pass (r2_proj_resize).

    ``size``: (mh, mw), the resized image.  ``interpolation``: "linear" is cv2's ``INTER_LINEAR`` sampling rule (pixel centres
    aligned, the taps clamped at the border: also torch's ``bilinear, align_corners=False``); "area" is the box mean, for
    factors H / mh and W / mw that are integers.  ``shift``: (sr, sc), the prepared image at (r, c) is the input at
    (r + sr, c + sc) and 0 beyond it: (5, 0) is the reference's ``proj_new[:-5] = proj[5:]``.  ``lo``: values below it become
    it before the resize (None: no clamp).  ``crop``: (r0, c0, oh, ow), the window of the resized image that is computed and
    returned (None: all of it).  ``out``: the result's tensor, allocated when None.  -> [oh,ow] or [V,oh,ow] float32."""
    # the arguments that do not depend on the projections first, then the projections, then what depends on their shape
    mh, mw = _pair(size, "size", 1)
    if mh * mw >= 2 ** 31:
        raise ValueError("a resized image of %d x %d is too large" % (mh, mw))
    if interpolation not in INTERPOLATIONS:
        raise ValueError("interpolation must be one of %s, got %r" % (sorted(INTERPOLATIONS), interpolation))
    sr, sc = _pair(shift, "shift")
    if max(abs(sr), abs(sc)) > 2 ** 30:
        raise ValueError("shift %r is out of range" % (shift,))
    lo = -math.inf if lo is None else float(lo)
    if math.isnan(lo):
        raise ValueError("lo must not be NaN")
    r0, c0, oh, ow = 0, 0, mh, mw
    if crop is not None:
        try:
            r0, c0, oh, ow = crop
            ok = all(int(v) == v for v in crop) and r0 >= 0 and c0 >= 0 and oh >= 1 and ow >= 1 and r0 + oh <= mh and c0 + ow <= mw
        except (TypeError, ValueError):
            ok = False
        if not ok:
            raise ValueError("crop must be (r0, c0, oh, ow), a non-empty window inside the %d x %d resized image, got %r"
                             % (mh, mw, crop))
        r0, c0, oh, ow = (int(v) for v in crop)
    p, single = _stack(projs)
    V, H, W = p.shape
    if interpolation == "area" and (H % mh or W % mw):
        raise ValueError("interpolation=\"area\" needs integer factors: %d x %d -> %d x %d has none" % (H, W, mh, mw))
    if V * oh * ow >= 2 ** 38:
        raise ValueError("the result [%d,%d,%d] is too large for one call: process it in batches of views" % (V, oh, ow))
    shape = (oh, ow) if single else (V, oh, ow)
    if out is None:
        out = torch.empty(shape, dtype=_F32, device=p.device)
    else:
        if not isinstance(out, torch.Tensor):
            raise _lib.R2HipError("out must be a GPU tensor: the MI355X kernels have no CPU fallback")
        require_gpu(out, "out")
        if tuple(out.shape) != shape or out.dtype != _F32 or not out.is_contiguous() or out.device != p.device:
            raise ValueError("out must be a contiguous float32 %s tensor on the projections' device" % (shape,))
    ws = None
    if interpolation == "linear":
        ws = workspace(int(_lib.lib().r2_proj_resize_workspace_bytes(mh, mw)), p.device, at_least=1)
    call("r2_proj_resize", p.device, V, H, W, p, sr, sc, lo, INTERPOLATIONS[interpolation], mh, mw, r0, c0, oh, ow, out, ws,
         0 if ws is None else ws.numel())
    return out


def _median(projs, size, conditional, threshold, want_mask):
    if isinstance(size, bool) or size not in (3, 5):
        raise ValueError("size must be 3 or 5, got %r" % (size,))
    threshold = float(threshold)
    if math.isnan(threshold) or threshold < 0:
        raise ValueError("threshold must be >= 0, got %r" % (threshold,))
    p, single = _stack(projs)
    V, H, W = p.shape
    dst = torch.empty_like(p)
    mask = torch.empty(p.shape, dtype=torch.uint8, device=p.device) if want_mask else None
    call("r2_proj_median", p.device, V, H, W, p, int(size), int(conditional), threshold, dst, mask)
    if single:
        dst, mask = dst[0], (mask[0] if want_mask else None)
    return dst, mask


def median_filter(projs, size=3):
    """``scipy.ndimage.median_filter(p, size=size, mode="nearest")`` of every projection (r2_proj_median): the median of the
    size x size window, ``size`` 3 or 5, with replicated borders; a NaN in a window counts as +inf.  -> float32, projs' shape."""
    return _median(projs, size, False, 0.0, False)[0]


def despeckle(projs, threshold, size=3, return_mask=False):
    """Replaces the pixels that are further than ``threshold`` from the median of their size x size window by that median, and
    every NaN pixel; all others come back bit for bit.  ``return_mask``: also the replaced pixels, a bool tensor of projs'
    shape.  -> despeckled, or (despeckled, mask)."""
    dst, mask = _median(projs, size, True, threshold, return_mask)
    return (dst, mask.bool()) if return_mask else dst


def _destripe(projs, size, method, want_dst, want_offsets):
    try:
        k = None if isinstance(size, bool) else operator.index(size)
    except TypeError:
        k = None
    if k is None or k % 2 != 1 or not 1 <= k <= 31:
        raise ValueError("size must be an odd integer in 1 .. 31, got %r" % (size,))
    size = k
    if method not in DESTRIPE_METHODS:
        raise ValueError("method must be one of %s, got %r" % (sorted(DESTRIPE_METHODS), method))
    if want_offsets and method != "mean":
        raise ValueError("the offsets are a by-product of method=\"mean\"; method=%r has none" % (method,))
    p, single = _stack(projs)
    V, H, W = p.shape
    if method == "sort" and V > destripe_max_views():
        raise ValueError("method=\"sort\" orders at most %d views, got %d: use method=\"mean\"" % (destripe_max_views(), V))
    if want_offsets and V == 0:
        raise ValueError("a stack without views has no offsets")
    ws = workspace(int(_lib.lib().r2_proj_destripe_workspace_bytes(V, H, W, DESTRIPE_METHODS[method])), p.device, at_least=1)
    dst = torch.empty_like(p) if want_dst else None
    offsets = torch.empty((H, W), dtype=_F32, device=p.device) if want_offsets else None
    if method == "sort":
        call("r2_proj_destripe_sort", p.device, V, H, W, p, size, dst, ws, ws.numel())
    else:
        call("r2_proj_destripe_mean", p.device, V, H, W, p, size, dst, offsets, ws, ws.numel())
    return (dst[0] if single and want_dst else dst), offsets


def destripe(projs, size=9, method="sort", return_offsets=False):
    """Removes the stripes of the sinogram, the rings of the reconstruction: what a detector pixel adds to every view.  Works
    along the view axis, so ``projs`` holds all views of the detector rows it covers ([H,W] is one view); rows are independent.
    ``size``: the odd width, 1 .. 31, of the median across detector columns.  ``method``: "sort" (r2_proj_destripe_sort: Vo,
    Atwood, Drakopoulos 2018, algorithm 3 -- every pixel's values sorted along the views, stably, a NaN as +inf, the sorted
    sinogram median-filtered across the columns, every value put back at the view its rank came from; handles partial and
    intensity-dependent stripes, at most ``destripe_max_views()`` views) or "mean" (r2_proj_destripe_mean: the mean over the views minus
    its median across the columns is the pixel's offset, which every view loses; full-length constant stripes only; a NaN
    spreads to its pixel in every view).  ``return_offsets``: with "mean", also the [H,W] offsets.
    -> float32 of projs' shape, or (that, offsets)."""
    dst, offsets = _destripe(projs, size, method, True, bool(return_offsets))
    return (dst, offsets) if return_offsets else dst


def stripe_offsets(projs, size=9):
    """The [H,W] offsets that ``destripe(projs, size, "mean")`` subtracts, alone: a diagnostic of the detector."""
    return _destripe(projs, size, "mean", False, True)[1]


def normalize(raw, flat, dark=None, eps=1e-6):
    """Measured intensities -> line integrals, ``-log((raw - dark) / (flat - dark))``, in plain torch: ``flat`` the open-beam
    image and ``dark`` the image without beam ([H,W], or anything that broadcasts against ``raw``).  The transmission is
    clamped to at least ``eps``, so a dead or a saturated pixel gives a finite value that ``despeckle`` can then remove."""
    for name, t in (("raw", raw), ("flat", flat)) + ((("dark", dark),) if dark is not None else ()):
        if not isinstance(t, torch.Tensor):
            raise _lib.R2HipError("%s must be a GPU tensor: the MI355X kernels have no CPU fallback" % name)
        require_gpu(t, name)
    raw, flat = raw.to(_F32), flat.to(_F32)
    if dark is not None:
        raw, flat = raw - dark.to(_F32), flat - dark.to(_F32)
    return -torch.log((raw / flat.clamp_min(eps)).clamp_min(eps))
