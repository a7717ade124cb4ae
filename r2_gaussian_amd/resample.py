"""Cubic-spline resampling of volumes on the MI355X (csrc/spline.hip; include/r2hip.h: r2_spline_prefilter, r2_spline_zoom,
r2_spline_sample): ``scipy.ndimage.zoom`` and ``map_coordinates`` for ``order=3, mode="nearest"``, and on top of them the
reference's raw-data helpers (data_generator/synthetic_dataset/process_raw_data.py) under their own names: ``resample``,
``resize``, ``crop_to_cube``, ``expand_to_cube``, ``reshape_vol``.  ``prepare.py`` is the command line on top of these.

Volumes are [nx,ny,nz] tensors on the GPU and so are the results: a host array raises, there is no CPU fallback.  Inputs of
another dtype or layout are converted to contiguous float32 first.  No host synchronisation.
"""
import numpy as np
import torch

from . import _lib
from ._boundary import call, f32c, require_gpu, workspace

_F32 = torch.float32
PAD = _lib.R2_SPLINE_PAD


def _order3(order):
    if order != 3:
        raise ValueError("only cubic splines (order=3) are implemented, got order=%r" % (order,))


def _volume(vol, name="vol"):
    if not isinstance(vol, torch.Tensor):
        raise _lib.R2HipError("%s must be a GPU tensor: the MI355X kernels have no CPU fallback" % name)
    require_gpu(vol, name)
    if vol.dim() != 3 or min(vol.shape) < 1:
        raise ValueError("%s must be a non-empty [nx,ny,nz] volume, got shape %s" % (name, tuple(vol.shape)))
    return f32c(vol.detach() if vol.requires_grad else vol)   # the tensor itself where it already is what the kernels read


def _padded(shape):
    p = tuple(int(n) + 2 * PAD for n in shape)
    if p[0] * p[1] * p[2] >= 2 ** 31:
        raise ValueError("a volume of %s is too large: its padded block must stay below 2^31 elements" % (tuple(shape),))
    return p


def spline_filter(vol, order=3):
    """The cubic B-spline coefficients of ``vol`` [nx,ny,nz] as ``zoom`` and ``map_coordinates`` use them: the volume
    edge-padded by 12 on every side and filtered along x, y and z -> [nx+24,ny+24,nz+24]."""
    _order3(order)
    vol = _volume(vol)
    coeffs = torch.empty(_padded(vol.shape), dtype=_F32, device=vol.device)
    call("r2_spline_prefilter", vol.device, *vol.shape, vol, coeffs)
    return coeffs


def output_shape(shape, zoom):
    """scipy's: ``int(round(n * f))`` per axis, Python's round (half to even)."""
    f = [zoom] * 3 if np.ndim(zoom) == 0 else list(zoom)
    if len(f) != 3:
        raise ValueError("zoom must be a number or a sequence of three, got %r" % (zoom,))
    return tuple(int(round(int(n) * float(v))) for n, v in zip(shape, f))


def _zoom_to(vol, shape, out=None):
    if min(shape) < 1:
        raise ValueError("the zoomed volume would be empty: shape %s" % (tuple(shape),))
    if shape[0] * shape[1] * shape[2] >= 2 ** 31:
        raise ValueError("the zoomed volume %s must stay below 2^31 voxels" % (tuple(shape),))
    if out is None:
        out = torch.empty(shape, dtype=_F32, device=vol.device)
    else:
        require_gpu(out, "out")
        if tuple(out.shape) != tuple(shape) or out.dtype != _F32 or not out.is_contiguous() or out.device != vol.device:
            raise ValueError("out must be a contiguous float32 %s tensor on vol's device" % (tuple(shape),))
    coeffs = spline_filter(vol)
    nbytes = int(_lib.lib().r2_spline_zoom_workspace_bytes(*shape))
    ws = workspace(nbytes, vol.device, at_least=1)
    call("r2_spline_zoom", vol.device, *vol.shape, coeffs, *shape, out, ws, ws.numel())
    return out


def zoom(vol, zoom, out=None, order=3):
    """``scipy.ndimage.zoom(vol, zoom, mode="nearest")``: ``zoom`` a factor or one per axis, the output shape
    ``int(round(n * f))``, its first and last nodes on the input's.  A factor of 1 is not a copy: the spline is filtered and
    evaluated at its nodes, as scipy does.  ``out``: the result's tensor, allocated when None.  -> out."""
    _order3(order)
    vol = _volume(vol)
    return _zoom_to(vol, output_shape(vol.shape, zoom), out)


def map_coordinates(vol, points, prefiltered=False, order=3):
    """``scipy.ndimage.map_coordinates(vol, points, order=3, mode="nearest")`` at ``points`` [..., 3], index coordinates of the
    volume (any real value; beyond the volume the edge value is approached).  ``prefiltered``: ``vol`` is ``spline_filter``'s
    result for the volume, to sample one volume many times.  A non-finite coordinate gives NaN.  -> [...] float32."""
    _order3(order)
    coeffs = _volume(vol)
    if prefiltered:
        if min(coeffs.shape) < 2 * PAD + 1:
            raise ValueError("prefiltered coefficients are [nx+24,ny+24,nz+24], got %s" % (tuple(coeffs.shape),))
    else:
        coeffs = spline_filter(coeffs)
    if not isinstance(points, torch.Tensor):
        raise _lib.R2HipError("points must be a GPU tensor: the MI355X kernels have no CPU fallback")
    require_gpu(points, "points")
    if points.dim() < 1 or points.shape[-1] != 3 or points.device != coeffs.device:
        raise ValueError("points must be [..., 3] on the volume's device, got %s on %s" % (tuple(points.shape), points.device))
    p = f32c(points.detach()).reshape(-1, 3)
    if p.shape[0] >= 2 ** 31:
        raise ValueError("too many points")
    out = torch.empty((p.shape[0],), dtype=_F32, device=coeffs.device)
    call("r2_spline_sample", coeffs.device, *(n - 2 * PAD for n in coeffs.shape), coeffs, p.shape[0], p, out)
    return out.reshape(points.shape[:-1])


# ---- the reference's helpers, under their names and with their arithmetic ----------------------------------------------------

def resample(vol, spacing, new_spacing=(1, 1, 1)):
    """Resample to ``new_spacing`` (the physical size stays, the voxel count changes) -> (volume, the spacing reached)."""
    vol = _volume(vol)
    spacing = np.array(list(spacing), dtype=np.float64)
    new_spacing = np.array(list(new_spacing), dtype=np.float64)
    shape = np.array(vol.shape)
    new_shape = np.round(shape * (spacing / new_spacing))
    real = new_shape / shape
    return zoom(vol, real), spacing / real


def resize(vol, target_size):
    """Zoom to ``target_size`` voxels along every axis; the input itself when every factor is 1."""
    vol = _volume(vol)
    f = tuple(target_size / int(n) for n in vol.shape)
    return zoom(vol, f) if any(v != 1.0 for v in f) else vol


def expand_to_cube(vol):
    """Zero-pad to a cube of the largest dimension, centred; an odd difference puts the extra voxel at the end."""
    vol = _volume(vol)
    m = max(vol.shape)
    out = torch.zeros((m, m, m), dtype=_F32, device=vol.device)
    s = [(m - int(n)) // 2 for n in vol.shape]
    out[s[0]:s[0] + vol.shape[0], s[1]:s[1] + vol.shape[1], s[2]:s[2] + vol.shape[2]] = vol
    return out


def crop_to_cube(vol):
    """The centred cube of the smallest dimension (offset ``(n - min) // 2``)."""
    vol = _volume(vol)
    m = min(vol.shape)
    s = [(int(n) - m) // 2 for n in vol.shape]
    return vol[s[0]:s[0] + m, s[1]:s[1] + m, s[2]:s[2] + m].contiguous()


def reshape_vol(vol, spacing, target_size, mode=None):
    """A scan of any shape and spacing -> ``target_size``^3: with ``mode`` "crop" or "expand" it is first resampled to unit
    spacing and made a cube; then (and with ``mode=None`` only this) it is resized."""
    vol = _volume(vol)
    if mode is not None:
        vol, _ = resample(vol, spacing, (1, 1, 1))
        if mode == "crop":
            vol = crop_to_cube(vol)
        elif mode == "expand":
            vol = expand_to_cube(vol)
        else:
            raise ValueError("Unsupported reshape mode!")
    return resize(vol, target_size)
