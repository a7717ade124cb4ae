"""Forward projection of a voxel volume without TIGRE: the counterpart of ``tigre.Ax`` as the reference's data generator
calls it (data_generator/synthetic_dataset/generate_data.py:47-69), on the MI355X kernel of csrc/projector.hip
(``r2_project_volume``).

Rays are the preimages of the pixel centres under the camera the rasterizer renders with (``scene.make_view``:
``world_view_transform``, ``tanfovx/y``, ``mode``), so a projection is registered to a rendered image of the same scene by
construction -- the forward half of what fdk.py does for the back-projection.  Pixel (r, c) has detector NDC
((2c+1)/W - 1, (2r+1)/H - 1), the inverse of ndc2Pix:

* cone (mode 1): from the camera centre along the view-space direction (ndc_x tanfovx, ndc_y tanfovy, 1), t >= 0;
* parallel (mode 0): the identity projection makes NDC view-space xy, so the ray passes through (ndc_x, ndc_y, .) along +z.
  As in fdk.py and the rasterizer, the parallel detector therefore spans view-space [-1, 1] whatever ``sDetector`` says, and
  ``offDetector`` is ignored by both beams.

The integrand is the trilinear interpolant of the volume (zero outside it), sampled at the midpoints of
n = max(1, ceil(L / accuracy)) equal pieces of the clipped chord (include/r2hip.h, r2_project_volume, states the contract).
That is ``projection_type="interpolated"``, the default.  ``projection_type="siddon"`` takes the ray-voxel intersection model
instead (csrc/projector_siddon.hip, ``r2_project_volume_siddon``): the exact integral of the piecewise-constant volume, voxel
(i,j,k) being a cube of constant value; it has no ``accuracy``.
"""
import numpy as np
import torch

from . import _lib
from . import scene as S
from ._C import _on_device, _require_gpu, _stream

_F32 = torch.float32
PROJECTION_TYPES = ("interpolated", "siddon")


def check_projection_type(projection_type):
    """-> ``projection_type``, or ValueError for anything but the two models."""
    if projection_type not in PROJECTION_TYPES:
        raise ValueError("projection_type must be one of %s, got %r" % (PROJECTION_TYPES, projection_type))
    return projection_type


def ray_params(views, sVoxel, center, nVoxel):
    """[V, 12] float32 ray parameters of ``views`` in voxel-index coordinates (include/r2hip.h: {a, p00, pu, pv}), derived in
    float64 from the views' float32 matrices."""
    nV = np.asarray(nVoxel, dtype=np.float64)
    d = np.asarray(sVoxel, dtype=np.float64) / nV
    corner = np.asarray(center, dtype=np.float64) - 0.5 * np.asarray(sVoxel, dtype=np.float64)
    out = np.empty((len(views), 12), dtype=np.float64)
    for i, v in enumerate(views):
        M = v.world_view_transform.detach().cpu().double().numpy()   # row vectors: view = [x, 1] M
        Rinv = np.linalg.inv(M[:3, :3])
        origin = -M[3, :3] @ Rinv                                  # world point of view-space (0, 0, 0)
        ex, ey, ez = Rinv[0], Rinv[1], Rinv[2]                     # world images of the view-space axes
        H, W = v.image_height, v.image_width
        tx, ty = float(v.tanfovx), float(v.tanfovy)
        if v.mode == 1:
            a = (origin - corner) / d - 0.5
            p00 = origin + ex * ((1.0 / W - 1.0) * tx) + ey * ((1.0 / H - 1.0) * ty) + ez
        else:
            a = ez / d
            p00 = origin + ex * (1.0 / W - 1.0) + ey * (1.0 / H - 1.0)
            tx = ty = 1.0
        out[i, 0:3] = a
        out[i, 3:6] = (p00 - corner) / d - 0.5
        out[i, 6:9] = ex * (2.0 * tx / W) / d
        out[i, 9:12] = ey * (2.0 * ty / H) / d
    return out.astype(np.float32)


def project_views(vol, views, sVoxel, center, accuracy=0.5, out=None, projection_type="interpolated"):
    """Line integrals of ``vol`` [nx,ny,nz] (GPU, the query() / voxelizer layout) along the rays of every pixel of ``views``
    (``scene.View`` list, one detector size): a GPU tensor [V,H,W] in scene units.  ``sVoxel`` / ``center``: the volume's
    extent and centre in the views' (scene) units.  No host synchronisation; ``out`` may be a preallocated [V,H,W] float32
    contiguous GPU tensor.  ``projection_type``: "interpolated" or "siddon" (which ignores ``accuracy``)."""
    check_projection_type(projection_type)
    _require_gpu(vol, "vol")
    if vol.dim() != 3:
        raise ValueError("vol must be a 3D array [nx,ny,nz], got shape %s" % (tuple(vol.shape),))
    if projection_type == "interpolated" and not accuracy > 0:
        raise ValueError("accuracy must be > 0, got %r" % (accuracy,))
    views = list(views)
    if not views:
        raise ValueError("no views to project")
    H, W = views[0].image_height, views[0].image_width
    if any((v.image_height, v.image_width) != (H, W) for v in views):
        raise ValueError("all views must share one detector size")
    if any(v.mode != views[0].mode for v in views):
        raise ValueError("all views must share one beam mode")
    if len(sVoxel) != 3 or len(center) != 3 or not all(s > 0 for s in sVoxel):
        raise ValueError("sVoxel must be three positive sizes and center three coordinates")
    v32 = vol if vol.dtype == _F32 and vol.is_contiguous() else vol.to(_F32).contiguous()
    nx, ny, nz = v32.shape
    V = len(views)
    if out is None:
        out = torch.empty((V, H, W), dtype=_F32, device=v32.device)
    elif (out.dtype != _F32 or not out.is_cuda or not out.is_contiguous() or tuple(out.shape) != (V, H, W)
          or out.device != v32.device):
        raise ValueError("out must be a contiguous float32 tensor [%d,%d,%d] on %s" % (V, H, W, v32.device))
    rays = torch.from_numpy(ray_params(views, sVoxel, center, (nx, ny, nz))).pin_memory().to(v32.device, non_blocking=True)
    d = [float(s) / n for s, n in zip(sVoxel, (nx, ny, nz))]
    L = _lib.lib()
    with _on_device(v32.device):
        if projection_type == "siddon":
            rc = L.r2_project_volume_siddon(V, H, W, rays.data_ptr(), int(views[0].mode == 1), nx, ny, nz, d[0], d[1], d[2],
                                            v32.data_ptr(), out.data_ptr(), _stream(v32.device))
        else:
            rc = L.r2_project_volume(V, H, W, rays.data_ptr(), int(views[0].mode == 1), nx, ny, nz, d[0], d[1], d[2],
                                     float(accuracy), v32.data_ptr(), out.data_ptr(), _stream(v32.device))
    _lib.check(rc, "r2_project_volume_siddon" if projection_type == "siddon" else "r2_project_volume")
    return out


def project(vol, angles, scanner_cfg, accuracy=None, device="cuda", projection_type="interpolated"):
    """``tigre.Ax(vol, geo, angles)[:, ::-1, :]`` as generate_data.py saves it: projections [V,H,W] (GPU tensor) of ``vol``
    [nx,ny,nz] at ``angles`` (radians) with the raw, unscaled scanner config (mode, DSD, DSO, nDetector [v, u], sDetector,
    sVoxel, offOrigin, accuracy), in the config's length units -- what dataset_readers.py:129 later multiplies by
    scene_scale.  Rows come in the rasterizer's order.  ``accuracy``: None takes the config's ``accuracy`` (0.5 if absent).
    ``projection_type``: "interpolated" or "siddon" (which ignores ``accuracy``)."""
    check_projection_type(projection_type)
    cfg = scanner_cfg
    v = torch.as_tensor(np.ascontiguousarray(vol) if isinstance(vol, np.ndarray) else vol)
    if v.dim() != 3:
        raise ValueError("vol must be a 3D array [nx,ny,nz], got shape %s" % (tuple(v.shape),))
    if tuple(int(n) for n in cfg["nVoxel"]) != tuple(v.shape):
        raise ValueError("vol shape %s differs from the config's nVoxel %s" % (tuple(v.shape), list(cfg["nVoxel"])))
    acc = cfg.get("accuracy", 0.5) if accuracy is None else accuracy
    if projection_type == "interpolated" and not acc > 0:
        raise ValueError("accuracy must be > 0, got %r" % (acc,))
    if not v.is_cuda:
        v = v.to(device)
    scale = 2.0 / max(cfg["sVoxel"])   # make_view works in the normalised scene (dataset_readers.py:62-76)
    H, W = (int(n) for n in cfg["nDetector"])
    views = [S.make_view(float(a), (H, W), cfg) for a in np.asarray(angles, dtype=np.float64).reshape(-1)]
    out = project_views(v, views, [s * scale for s in cfg["sVoxel"]], [o * scale for o in cfg["offOrigin"]], acc,
                        projection_type=projection_type)
    return out.mul_(1.0 / scale)
