"""Conditioning of measured projections on the MI355X (csrc/projections.hip; include/r2hip.h: r2_proj_resize,
r2_proj_median): what the reference's real-data converter does to a measured stack with cv2 and numpy -- lower clamp, row
shift, ``cv2.resize``, crop -- as one fused pass, and a median filter against the isolated outliers of measured data (zingers,
hot pixels, NaN read-outs), which ``weights.fill_unmeasured`` only handles once they are known.  ``prepare_real.py`` is the
command line on top of these.

Projections are [H,W] or [V,H,W] tensors on the GPU and so are the results: a host array raises, there is no CPU fallback.
Inputs of another dtype or layout are converted to contiguous float32 first.  No host synchronisation.
"""
import math

import torch

from . import _lib
from ._boundary import call, f32c, require_gpu, workspace

_F32 = torch.float32
INTERPOLATIONS = {"linear": 0, "area": 1}


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
