"""Direct volume rendering without pyvista or a monitor: the counterpart of ``plotter.add_volume(volume, cmap="viridis",
opacity="linear", clim=[0, 1])`` as the reference's scripts/plot_volume.py (Fig. 1 of the paper) and
data_generator/check_volume.py call it, on the MI355X kernels of csrc/volume_render.hip (``r2_render_volume``,
``r2_render_volume_mip``, ``r2_volume_bricks``; include/r2hip.h states the contract).

The renderer walks the rays of projector.py -- the same [V,12] ray parameters in voxel-index coordinates, the same clip,
sample count and trilinear samples -- and composites them front to back through a transfer function instead of summing them:

* ``transfer_function`` makes the [K,4] table (r, g, b, extinction) from a colormap and an opacity function;
* ``look_at_rays`` / ``orbit_rays`` place a free camera, ``view_rays`` renders the volume as the scanner sees it;
* ``render_volume`` is the emission-absorption image [V,H,W,4] (premultiplied colour, opacity), ``mip`` the maximum
  intensity projection [V,H,W]; ``volume_bricks`` is the min/max table that lets both pass over empty space, with the same
  bits as without it;
* ``over``, ``to_rgb8`` and ``write_png`` (zlib and struct only) turn the result into a picture.

The driver reproduces plot_volume.py's picture -- half the volume cut away along x, viridis, linear opacity, clim [0, 1], a
window 800 wide and 1000 high, the script's camera direction -- from a .npy volume:

    python -m r2_gaussian_amd.volume_render --volume vol_gt.npy --out volume.png [--scanner cfg.yml | --meta meta_data.json]
        [--cmap viridis] [--clim 0 1] [--opacity linear] [--unit U] [--size 1000 800] [--azimuth A --elevation E
        --distance D --fov F] [--cut {x,y,z} FRACTION] [--mip] [--turntable N]

The opacity unit.  An opacity ``a`` of the transfer function is what a path of world length ``unit`` through that value
absorbs: extinction = -log(1 - a) / unit.  The driver's default is the volume's diagonal divided by its mean side in voxels,
the convention of pyvista's default opacity unit distance; it is a convention for comparable pictures, not a bit-match to
pyvista (whose mapper samples and blends differently).
"""
import struct
import zlib

import numpy as np
import torch

from . import _lib
from . import projector as P
from ._boundary import _F32, call, f32c

MAX_K = 1024                      # include/r2hip.h: the table lives in LDS
_A_MAX = 1.0 - 2.0 ** -24         # the largest opacity below 1: a finite extinction
# plot_volume.py's camera (cpos) relative to its 256^3 volume: direction of the eye from the centre, and its distance in
# units of the largest side
AZIMUTH, ELEVATION, DISTANCE, FOV = 210.0, 16.0, 2.75, 30.0


# ---- the transfer function ---------------------------------------------------------------------------------------------------

def _resample(table, K):
    """[N, C] -> [K, C]: linear between the rows, both ends kept."""
    table = np.asarray(table, dtype=np.float64)
    if table.shape[0] == K:
        return table
    x = np.linspace(0.0, 1.0, K)
    xp = np.linspace(0.0, 1.0, table.shape[0])
    return np.stack([np.interp(x, xp, table[:, c]) for c in range(table.shape[1])], 1)


def _colours(cmap, K):
    """-> ([K,3] float64 colours, [K] opacities or None) of a colormap name or array."""
    if isinstance(cmap, str):
        if cmap == "gray":
            return np.repeat(np.linspace(0.0, 1.0, K)[:, None], 3, 1), None
        if cmap == "viridis":
            from ._viridis import VIRIDIS
            return _resample(np.asarray(VIRIDIS), K), None
        try:
            import matplotlib
            cm = matplotlib.colormaps[cmap]
        except (ImportError, KeyError):
            raise ValueError("cmap %r: 'gray' and 'viridis' are built in, other names need matplotlib to know them" % (cmap,))
        return np.asarray(cm(np.linspace(0.0, 1.0, K)), dtype=np.float64)[:, :3], None
    table = np.asarray(cmap, dtype=np.float64)
    if table.ndim != 2 or table.shape[1] not in (3, 4) or table.shape[0] < 2 or not np.isfinite(table).all():
        raise ValueError("cmap must be 'gray', 'viridis', a matplotlib name or a finite [N,3] / [N,4] array with N >= 2")
    table = _resample(table, K)
    return table[:, :3], (table[:, 3] if table.shape[1] == 4 else None)


def transfer_function(cmap="viridis", opacity="linear", unit=None, K=256):
    """The [K,4] float32 table (r, g, b, ext) that ``render_volume`` reads, row j standing at the value
    clim[0] + j (clim[1] - clim[0]) / (K - 1).

    cmap: "gray", "viridis" (the committed 256-row table), any matplotlib name where matplotlib imports, or an [N,3] / [N,4]
    array of colours in [0, 1], resampled linearly to K rows.  opacity: "linear" (a ramp 0 -> 1 over the window: pyvista's
    opacity="linear"), a number (the same everywhere), or a sequence of opacities in [0, 1], resampled linearly to K (one of
    K entries is taken as it is); None takes the fourth column of an [N,4] cmap.  unit (required): the world length over which
    a value of opacity a absorbs the fraction a, ext = -log1p(-min(a, 1 - 2^-24)) / unit in float64 (the module docstring
    says how the driver picks it)."""
    K = int(K)
    if not 2 <= K <= MAX_K:
        raise ValueError("K must be in [2, %d], got %r" % (MAX_K, K))
    if unit is None or not (float(unit) > 0 and np.isfinite(float(unit))):
        raise ValueError("unit must be a positive, finite world length, got %r" % (unit,))
    rgb, a4 = _colours(cmap, K)
    if opacity is None:
        if a4 is None:
            raise ValueError("opacity=None needs an [N,4] cmap whose fourth column is the opacity")
        a = a4
    elif isinstance(opacity, str):
        if opacity != "linear":
            raise ValueError("opacity must be 'linear', a number or a sequence, got %r" % (opacity,))
        a = np.linspace(0.0, 1.0, K)
    elif np.ndim(opacity) == 0:
        a = np.full(K, float(opacity))
    else:
        a = np.asarray(opacity, dtype=np.float64)
        if a.ndim != 1 or a.shape[0] < 2:
            raise ValueError("an opacity sequence must be 1D with at least 2 entries, got shape %s" % (a.shape,))
        a = _resample(a[:, None], K)[:, 0]
    if not (np.isfinite(a).all() and (a >= 0).all() and (a <= 1).all()):
        raise ValueError("opacities must lie in [0, 1]")
    ext = -np.log1p(-np.minimum(a, _A_MAX)) / float(unit)
    return np.concatenate([rgb, ext[:, None]], 1).astype(np.float32)


# ---- cameras -------------------------------------------------------------------------------------------------------------------

def look_at_rays(eye, target, up, H, W, sVoxel, center, nVoxel, fov_y=None, ortho_height=None):
    """([1,12] float32 ray parameters in voxel-index coordinates, cone) of a camera at ``eye`` looking at ``target`` (world
    units, the volume spanning ``center`` +- ``sVoxel`` / 2), image rows running against ``up``.  Derived in float64 by the
    rule of ``projector.ray_params``: pixel (r, c) has NDC ((2c+1)/W - 1, (2r+1)/H - 1), pixels are square.  Exactly one of
    ``fov_y`` (degrees: a perspective camera, cone = True, the rays leave ``eye``) and ``ortho_height`` (world height of the
    image: parallel rays through the image plane at ``eye``, cone = False) must be given."""
    if (fov_y is None) == (ortho_height is None):
        raise ValueError("give exactly one of fov_y (perspective) and ortho_height (orthographic)")
    H, W = int(H), int(W)
    if H < 1 or W < 1:
        raise ValueError("H and W must be >= 1, got %r x %r" % (H, W))
    P._check_extent(sVoxel, center)
    nV = np.asarray(nVoxel, dtype=np.float64)
    if nV.shape != (3,) or not (nV >= 1).all():
        raise ValueError("nVoxel must be three positive sizes, got %r" % (nVoxel,))
    eye, target, up = (np.asarray(v, dtype=np.float64).reshape(-1) for v in (eye, target, up))
    if eye.shape != (3,) or target.shape != (3,) or up.shape != (3,):
        raise ValueError("eye, target and up must be three coordinates each")
    ez = target - eye
    ex = np.cross(ez, up)
    if not (np.linalg.norm(ez) > 0 and np.linalg.norm(ex) > 0):
        raise ValueError("the camera needs eye != target and an up that is not along the viewing direction")
    ez, ex = ez / np.linalg.norm(ez), ex / np.linalg.norm(ex)
    ey = np.cross(ez, ex)                                       # image rows run down: against up
    d = np.asarray(sVoxel, dtype=np.float64) / nV
    corner = np.asarray(center, dtype=np.float64) - 0.5 * np.asarray(sVoxel, dtype=np.float64)
    out = np.empty((1, 12), dtype=np.float64)
    if fov_y is not None:
        if not 0 < float(fov_y) < 180:
            raise ValueError("fov_y must be in (0, 180) degrees, got %r" % (fov_y,))
        ty = np.tan(np.radians(float(fov_y)) / 2)
        tx = ty * W / H
        out[0, 0:3] = (eye - corner) / d - 0.5
        p00 = eye + ex * ((1.0 / W - 1.0) * tx) + ey * ((1.0 / H - 1.0) * ty) + ez
    else:
        if not float(ortho_height) > 0:
            raise ValueError("ortho_height must be > 0, got %r" % (ortho_height,))
        ty = float(ortho_height) / 2
        tx = ty * W / H
        out[0, 0:3] = ez / d
        p00 = eye + ex * ((1.0 / W - 1.0) * tx) + ey * ((1.0 / H - 1.0) * ty)
    out[0, 3:6] = (p00 - corner) / d - 0.5
    out[0, 6:9] = ex * (2.0 * tx / W) / d
    out[0, 9:12] = ey * (2.0 * ty / H) / d
    return out.astype(np.float32), fov_y is not None


def orbit_rays(azimuths, elevation, distance, H, W, sVoxel, center, nVoxel, fov_y=FOV, up=(0.0, 0.0, 1.0)):
    """[V,12] perspective rays (cone = True) of a turntable: one camera per azimuth (degrees, about the world z axis through
    ``center``), all at ``elevation`` degrees above the xy plane and ``distance`` (world units) from ``center``, looking at
    it."""
    c = np.asarray(center, dtype=np.float64)
    el = np.radians(float(elevation))
    rays = []
    for az in np.asarray(azimuths, dtype=np.float64).reshape(-1):
        a = np.radians(az)
        eye = c + float(distance) * np.array([np.cos(el) * np.cos(a), np.cos(el) * np.sin(a), np.sin(el)])
        rays.append(look_at_rays(eye, c, up, H, W, sVoxel, center, nVoxel, fov_y=fov_y)[0])
    if not rays:
        raise ValueError("no azimuths")
    return np.concatenate(rays, 0)


def view_rays(views, sVoxel, center, nVoxel):
    """``projector.ray_params``: render the volume as the scanner sees it (``scene.View`` list -> [V,12]; cone is
    ``views[0].mode == 1``)."""
    return P.ray_params(views, sVoxel, center, nVoxel)


# ---- the kernels ---------------------------------------------------------------------------------------------------------------

def _brick_shape(n):
    B = _lib.R2_RENDER_BRICK
    return tuple((int(m) + B - 1) // B for m in n) + (2,)


def volume_bricks(vol):
    """The min/max table [bx,by,bz,2] (GPU, float32) of ``vol`` [nx,ny,nz] (GPU) over bricks of 8 cells a side
    (``r2_volume_bricks``): independent of any transfer function, reusable for as long as ``vol`` is unchanged.  No host
    synchronisation."""
    P._check_operand(vol, "vol", "a 3D array [nx,ny,nz]", "interpolated")
    v32 = f32c(vol)
    out = torch.empty(_brick_shape(v32.shape), dtype=_F32, device=v32.device)
    call("r2_volume_bricks", v32.device, *v32.shape, v32, out)
    return out


def _bricks_for(bricks, v32):
    """``bricks`` as the kernels take it: True builds the table, a tensor from ``volume_bricks`` is checked and reused,
    False / None is no table."""
    if bricks is None or bricks is False:
        return None
    if bricks is True:
        return volume_bricks(v32)
    shape = _brick_shape(v32.shape)
    if (not isinstance(bricks, torch.Tensor) or bricks.dtype != _F32 or not bricks.is_cuda or not bricks.is_contiguous()
            or bricks.device != v32.device or tuple(bricks.shape) != shape):
        raise ValueError("bricks must be True, False or the contiguous float32 tensor %s of volume_bricks on %s"
                         % (list(shape), v32.device))
    return bricks


def _image_size(H, W):
    H, W = int(H), int(W)
    if H < 1 or W < 1:
        raise ValueError("H and W must be >= 1, got %r x %r" % (H, W))
    return H, W


def _checked_lut(lut):
    """The table as a float32 [K,4] array or tensor; a host table's values are checked (a device table's are the caller's)."""
    t = lut if isinstance(lut, torch.Tensor) else torch.from_numpy(np.array(lut, dtype=np.float32))   # a copy: a read-only table is taken too
    if t.dim() != 2 or t.shape[1] != 4 or not 2 <= t.shape[0] <= MAX_K:
        raise ValueError("lut must be [K,4] = (r, g, b, ext) with K in [2, %d], got shape %s" % (MAX_K, tuple(t.shape)))
    if not t.is_cuda and not (bool(torch.isfinite(t).all()) and bool((t[:, 3] >= 0).all())):
        raise ValueError("lut must be finite with ext >= 0")
    return t


def _device_lut(t, device):
    if t.is_cuda:
        if t.device != device:
            raise ValueError("lut is on %s, the volume on %s" % (t.device, device))
        return f32c(t)
    return f32c(t).pin_memory().to(device, non_blocking=True)


def _output(out, shape, device):
    if out is None:
        return torch.empty(shape, dtype=_F32, device=device)
    if (not isinstance(out, torch.Tensor) or out.dtype != _F32 or not out.is_cuda or not out.is_contiguous()
            or out.device != device or tuple(out.shape) != tuple(shape)):
        raise ValueError("out must be a contiguous float32 tensor %s on %s" % (list(shape), device))
    return out


def render_volume(vol, rays, cone, H, W, dVoxel, lut, clim, accuracy=0.5, t_stop=2.0 ** -10, bricks=True, out=None):
    """The emission-absorption image [V,H,W,4] (GPU, float32: premultiplied r, g, b and the opacity) of ``vol`` [nx,ny,nz]
    (GPU) along ``rays`` [V,12] (``cone`` as in ``projector.project_rays``, whose samples these are), under the transfer
    function ``lut`` [K,4] (``transfer_function``) over the window ``clim`` = (lo, hi); ``dVoxel`` scales index lengths to the
    world lengths the table's extinction is per.  A ray stops after the first sample that leaves its transmittance below
    ``t_stop`` (0: never).  ``bricks``: True builds the min/max table and passes over empty space, a tensor from
    ``volume_bricks`` reuses it, False / None visits every sample; the image is the same bits either way.  Arguments are
    checked (ValueError) before anything is launched; no host synchronisation; ``out`` may be a preallocated contiguous
    float32 GPU tensor [V,H,W,4]."""
    H, W = _image_size(H, W)
    P.check_accuracy(accuracy, "interpolated")
    dVoxel = P._voxel_sizes(dVoxel)
    lut = _checked_lut(lut)
    if len(clim) != 2 or not (np.isfinite(float(clim[0])) and np.isfinite(float(clim[1])) and float(clim[1]) > float(clim[0])):
        raise ValueError("clim must be (lo, hi), finite with hi > lo, got %r" % (clim,))
    if not 0.0 <= float(t_stop) < 1.0:
        raise ValueError("t_stop must be in [0, 1), got %r" % (t_stop,))
    P._check_operand(vol, "vol", "a 3D array [nx,ny,nz]", "interpolated")
    rays = P.device_rays(rays, vol.device)
    out = _output(out, (rays.shape[0], H, W, 4), vol.device)
    v32 = f32c(vol)
    table = _bricks_for(bricks, v32)
    lut = _device_lut(lut, vol.device)
    call("r2_render_volume", vol.device, rays.shape[0], H, W, rays, int(bool(cone)), *v32.shape, *dVoxel, float(accuracy), v32,
         table, lut.shape[0], lut, float(clim[0]), float(clim[1]), float(t_stop), out)
    return out


def mip(vol, rays, cone, H, W, dVoxel, accuracy=0.5, bricks=True, out=None):
    """The maximum intensity projection [V,H,W] (GPU, float32) of ``vol`` over the samples ``render_volume`` takes; a ray
    that misses the volume gives 0.  ``bricks`` and ``out`` ([V,H,W]) as there: the same bits with and without the table."""
    H, W = _image_size(H, W)
    P.check_accuracy(accuracy, "interpolated")
    dVoxel = P._voxel_sizes(dVoxel)
    P._check_operand(vol, "vol", "a 3D array [nx,ny,nz]", "interpolated")
    rays = P.device_rays(rays, vol.device)
    out = _output(out, (rays.shape[0], H, W), vol.device)
    v32 = f32c(vol)
    table = _bricks_for(bricks, v32)
    call("r2_render_volume_mip", vol.device, rays.shape[0], H, W, rays, int(bool(cone)), *v32.shape, *dVoxel, float(accuracy),
         v32, table, out)
    return out


# ---- pictures ------------------------------------------------------------------------------------------------------------------

def over(rgba, background=(1.0, 1.0, 1.0)):
    """The premultiplied image [..., 4] over an opaque background colour: rgb + (1 - alpha) background -> [..., 3]."""
    if rgba.shape[-1] != 4:
        raise ValueError("rgba must be [..., 4], got shape %s" % (tuple(rgba.shape),))
    bg = torch.as_tensor(background, dtype=rgba.dtype, device=rgba.device).reshape(-1)
    if bg.numel() != 3:
        raise ValueError("background must be three components, got %r" % (background,))
    return rgba[..., :3] + (1.0 - rgba[..., 3:4]) * bg


def to_rgb8(rgb):
    """[..., 3] (or [...] grey) in [0, 1], tensor or array -> uint8 numpy, rounded to nearest and clamped."""
    a = rgb.detach().cpu().numpy() if isinstance(rgb, torch.Tensor) else np.asarray(rgb)
    a = np.nan_to_num(a.astype(np.float64), nan=0.0)
    return np.floor(np.clip(a, 0.0, 1.0) * 255.0 + 0.5).astype(np.uint8)


def write_png(path, rgb8):
    """An 8-bit PNG of ``rgb8``, uint8 [H,W,3] (truecolour) or [H,W] (greyscale), with zlib and struct only."""
    a = np.asarray(rgb8)
    if a.dtype != np.uint8 or not (a.ndim == 2 or (a.ndim == 3 and a.shape[2] == 3)) or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError("write_png takes uint8 [H,W,3] or [H,W], got %s %s" % (a.dtype, a.shape))
    H, W = a.shape[:2]
    # every scanline starts with its filter type, 0: none
    raw = np.concatenate([np.zeros((H, 1), np.uint8), np.ascontiguousarray(a).reshape(H, -1)], 1).tobytes()

    def chunk(kind, data):
        return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xFFFFFFFF)

    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n")
        f.write(chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, 2 if a.ndim == 3 else 0, 0, 0, 0)))
        f.write(chunk(b"IDAT", zlib.compress(raw, 6)))
        f.write(chunk(b"IEND", b""))


def default_unit(sVoxel, nVoxel):
    """The driver's opacity unit: the volume's diagonal divided by its mean side in voxels (the module docstring)."""
    return float(np.sqrt(np.sum(np.asarray(sVoxel, dtype=np.float64) ** 2)) / np.mean(np.asarray(nVoxel, dtype=np.float64)))


def picture(vol, sVoxel=None, center=None, size=(1000, 800), cmap="viridis", clim=(0.0, 1.0), opacity="linear", unit=None,
            azimuth=AZIMUTH, elevation=ELEVATION, distance=DISTANCE, fov=FOV, cut=("x", 0.5), use_mip=False,
            background=(1.0, 1.0, 1.0), accuracy=0.5):
    """uint8 pictures [V,H,W,3] of ``vol`` [nx,ny,nz] (GPU) at plot_volume.py's defaults: ``size`` = (H, W); the camera
    ``distance`` largest sides away from the centre at ``azimuth`` / ``elevation`` degrees (a sequence of azimuths: one
    picture each); ``cut`` = (axis, fraction) zeroes that leading fraction of the volume along the axis (None: nothing) to
    show the inside; ``use_mip``: the maximum intensity through the colormap instead of the compositing.  ``sVoxel`` /
    ``center``: the volume's world extent (default: the largest side 2 long, centred at 0)."""
    P._check_operand(vol, "vol", "a 3D array [nx,ny,nz]", "interpolated")
    n = tuple(vol.shape)
    if sVoxel is None:
        sVoxel = [2.0 * m / max(n) for m in n]
    if center is None:
        center = [0.0, 0.0, 0.0]
    H, W = _image_size(*size)
    unit = default_unit(sVoxel, n) if unit is None else unit
    lut = transfer_function(cmap, opacity, unit)
    v = f32c(vol)
    if cut is not None and float(cut[1]) > 0:
        if cut[0] not in ("x", "y", "z") or not float(cut[1]) <= 1:
            raise ValueError("cut must be (axis in 'xyz', fraction in [0, 1]), got %r" % (cut,))
        v = v.clone()
        ax = "xyz".index(cut[0])
        v.narrow(ax, 0, int(n[ax] * float(cut[1]))).zero_()
    rays = orbit_rays(azimuth, elevation, float(distance) * max(sVoxel), H, W, sVoxel, center, n, fov_y=fov)
    dVoxel = [float(s) / m for s, m in zip(sVoxel, n)]
    if use_mip:
        m = mip(v, rays, True, H, W, dVoxel, accuracy)
        x = ((m - float(clim[0])) / (float(clim[1]) - float(clim[0]))).clamp_(0.0, 1.0).cpu().numpy()
        K = lut.shape[0]
        xi = x * (K - 1)
        i = np.minimum(xi.astype(np.int64), K - 2)
        rgb = lut[i, :3] + (xi - i)[..., None] * (lut[i + 1, :3] - lut[i, :3])
        return to_rgb8(rgb)
    return to_rgb8(over(render_volume(v, rays, True, H, W, dVoxel, lut, clim, accuracy), background))


# ---- the driver ----------------------------------------------------------------------------------------------------------------

def _extent(args):
    """(center, sVoxel, nVoxel) of the raw scanner config of --scanner (YAML) or --meta (meta_data.json), or None."""
    if args.scanner:
        import yaml
        with open(args.scanner, "r") as f:
            cfg = yaml.safe_load(f)
    elif args.meta:
        import json
        with open(args.meta, "r", encoding="utf-8") as f:
            cfg = json.load(f)["scanner"]
    else:
        return None
    return [float(c) for c in cfg["offOrigin"]], [float(s) for s in cfg["sVoxel"]], [int(n) for n in cfg["nVoxel"]]


def parser():
    import argparse
    ap = argparse.ArgumentParser(description="A picture of a volume by direct volume rendering: plot_volume.py without a monitor")
    ap.add_argument("--volume", type=str, required=True, help="a volume [nx,ny,nz] as .npy")
    ap.add_argument("--out", type=str, required=True, help="the picture, .png (--turntable N: name_000.png ...)")
    ext = ap.add_mutually_exclusive_group()
    ext.add_argument("--scanner", type=str, help="scanner configuration (YAML): nVoxel, sVoxel, offOrigin give the extent")
    ext.add_argument("--meta", type=str, help="a case's meta_data.json: its scanner configuration gives the extent")
    ap.add_argument("--cmap", type=str, default="viridis", help="gray, viridis, or a matplotlib name where it is installed")
    ap.add_argument("--clim", type=float, nargs=2, default=[0.0, 1.0], metavar=("LO", "HI"))
    ap.add_argument("--opacity", type=str, default="linear", help="linear, or one number in [0, 1]")
    ap.add_argument("--unit", type=float, default=None,
                    help="world length over which an opacity absorbs (default: the diagonal / the mean side in voxels)")
    ap.add_argument("--size", type=int, nargs=2, default=[1000, 800], metavar=("H", "W"), help="rows and columns")
    ap.add_argument("--azimuth", type=float, default=AZIMUTH, help="degrees about z (the first frame of a turntable)")
    ap.add_argument("--elevation", type=float, default=ELEVATION, help="degrees above the xy plane")
    ap.add_argument("--distance", type=float, default=DISTANCE, help="from the centre, in largest sides of the volume")
    ap.add_argument("--fov", type=float, default=FOV, help="vertical field of view, degrees")
    ap.add_argument("--cut", nargs=2, default=["x", "0.5"], metavar=("AXIS", "FRACTION"),
                    help="zero this leading fraction along x, y or z to show the inside (fraction 0: the whole volume)")
    ap.add_argument("--mip", action="store_true", help="maximum intensity projection through the colormap")
    ap.add_argument("--turntable", type=int, default=0, metavar="N", help="N pictures, a full turn about z")
    ap.add_argument("--background", type=float, nargs=3, default=[1.0, 1.0, 1.0], metavar=("R", "G", "B"))
    ap.add_argument("--accuracy", type=float, default=0.5, help="samples are at most this many voxels apart")
    ap.add_argument("--device", type=str, default="cuda")
    return ap


def main(argv=None):
    import os
    ap = parser()
    args = ap.parse_args(argv)
    if not args.out.lower().endswith(".png"):
        ap.error("--out must end in .png")
    if args.cut[0] not in ("x", "y", "z"):
        ap.error("--cut takes an axis x, y or z and a fraction")
    try:
        opacity = args.opacity if args.opacity == "linear" else float(args.opacity)
        cut = (args.cut[0], float(args.cut[1]))
    except ValueError:
        ap.error("--opacity is linear or a number, --cut's fraction a number")
    if args.turntable < 0:
        ap.error("--turntable must be >= 0")
    vol = torch.from_numpy(np.load(args.volume).astype(np.float32)).to(args.device)
    if vol.dim() != 3:
        ap.error("the volume must be 3D, got shape %s" % (list(vol.shape),))
    extent = _extent(args)
    if extent is not None and list(vol.shape) != extent[2]:
        ap.error("the volume is %s, the scanner configuration's nVoxel %s" % (list(vol.shape), extent[2]))
    center, sVoxel = (None, None) if extent is None else extent[:2]
    N = args.turntable
    az = [args.azimuth + 360.0 * i / N for i in range(N)] if N else [args.azimuth]
    names = ["%s_%03d.png" % (args.out[:-4], i) for i in range(N)] if N else [args.out]
    # one view per launch: a turntable's pictures leave the device one at a time
    for a, name in zip(az, names):
        img = picture(vol, sVoxel, center, args.size, args.cmap, args.clim, opacity, args.unit, [a], args.elevation,
                      args.distance, args.fov, cut, args.mip, args.background, args.accuracy)[0]
        write_png(name, img)
        print("%s: %d x %d, azimuth %g" % (os.path.basename(name), img.shape[1], img.shape[0], a))


if __name__ == "__main__":
    main()
