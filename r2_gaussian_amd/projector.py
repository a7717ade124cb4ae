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

Both directions of both models live here: the exact transposes ``r2_backproject_volume`` and ``r2_backproject_volume_siddon``
(csrc/backprojector.hip, csrc/backprojector_siddon.hip on the gather of csrc/voxel_gather.hpp), the rays-level pair
``project_rays`` / ``backproject_rays`` for detectors a camera cannot describe, and ``Operator``, the pair in the raw scanner
config's units that the iterative reconstructions (recon.py) are built on.
"""
import numpy as np
import torch

from . import _lib
from . import scene as S
from ._boundary import _F32, call, f32c, require_gpu

PROJECTION_TYPES = ("interpolated", "siddon")
# (direction, projection_type) -> the C function and whether it takes ``accuracy``
_ENTRY_POINTS = {
    ("project", "interpolated"): ("r2_project_volume", True),
    ("project", "siddon"): ("r2_project_volume_siddon", False),
    ("backproject", "interpolated"): ("r2_backproject_volume", True),
    ("backproject", "siddon"): ("r2_backproject_volume_siddon", False),
}


# ---- the checks, one of each ------------------------------------------------------------------------------------------------

def check_projection_type(projection_type):
    """-> ``projection_type``, or ValueError for anything but the two models."""
    if projection_type not in PROJECTION_TYPES:
        raise ValueError("projection_type must be one of %s, got %r" % (PROJECTION_TYPES, projection_type))
    return projection_type


def check_accuracy(accuracy, projection_type):
    """ValueError unless ``accuracy`` > 0; "siddon" has none and does not look at it."""
    if projection_type == "interpolated" and not accuracy > 0:
        raise ValueError("accuracy must be > 0, got %r" % (accuracy,))


def check_views(views):
    """-> (list of views, H, W), or ValueError unless there is a view and all share one detector size and one beam mode."""
    views = list(views)
    if not views:
        raise ValueError("no views")
    H, W = views[0].image_height, views[0].image_width
    if any((v.image_height, v.image_width) != (H, W) for v in views):
        raise ValueError("all views must share one detector size")
    if any(v.mode != views[0].mode for v in views):
        raise ValueError("all views must share one beam mode")
    return views, H, W


def _check_extent(sVoxel, center):
    if len(sVoxel) != 3 or len(center) != 3 or not all(s > 0 for s in sVoxel):
        raise ValueError("sVoxel must be three positive sizes and center three coordinates")


def _check_operand(t, name, layout, projection_type):
    """The model first, then the GPU requirement, then the operand's rank."""
    check_projection_type(projection_type)
    require_gpu(t, name)
    if t.dim() != 3:
        raise ValueError("%s must be %s, got shape %s" % (name, layout, tuple(t.shape)))


def device_rays(rays, device):
    """[V,12] ray parameters as a contiguous float32 tensor on ``device``: host rays go through pinned memory without a
    host synchronisation, rays already there are taken as they are."""
    rays = torch.as_tensor(rays)
    if rays.dim() != 2 or rays.shape[1] != 12:
        raise ValueError("rays must be [V,12], got shape %s" % (tuple(rays.shape),))
    if rays.is_cuda:
        if rays.device != device:
            raise ValueError("rays are on %s, the operand on %s" % (rays.device, device))
        return f32c(rays)
    return f32c(rays).pin_memory().to(device, non_blocking=True)


def _output(out, shape, device, layout):
    """``out`` checked against ``shape`` (None: any 3D shape), or a new tensor of that shape."""
    if out is None:
        return torch.empty(shape, dtype=_F32, device=device)
    if (not isinstance(out, torch.Tensor) or out.dtype != _F32 or not out.is_cuda or not out.is_contiguous() or out.dim() != 3
            or out.device != device or (shape is not None and tuple(out.shape) != tuple(shape))):
        raise ValueError("out must be a contiguous float32 tensor %s on %s" % (layout, device))
    return out


def _volume_output(out, nVoxel, device):
    """The volume an adjoint writes: ``out``, of the shape ``nVoxel`` where that is given, or a new one of that shape."""
    if nVoxel is not None:
        if len(nVoxel) != 3 or not all(int(n) > 0 for n in nVoxel):
            raise ValueError("nVoxel must be three positive sizes, got %r" % (nVoxel,))
        nVoxel = tuple(int(n) for n in nVoxel)
    elif out is None:
        raise ValueError("give the volume's shape: nVoxel (three positive sizes) or out")
    return _output(out, nVoxel, device, "[nx,ny,nz]")


def _voxel_sizes(dVoxel):
    if len(dVoxel) != 3 or not all(d > 0 for d in dVoxel):
        raise ValueError("dVoxel must be three positive sizes, got %r" % (dVoxel,))
    return [float(d) for d in dVoxel]


# ---- the one launch site ------------------------------------------------------------------------------------------------------

def _launch(direction, projection_type, rays, cone, H, W, nVoxel, dVoxel, accuracy, src, dst):
    """``dst`` = A ``src`` ("project") or A^T ``src`` ("backproject") on checked, contiguous float32 GPU operands."""
    name, takes_accuracy = _ENTRY_POINTS[direction, projection_type]
    args = [rays.shape[0], H, W, rays, int(bool(cone))] + list(nVoxel) + list(dVoxel)
    if takes_accuracy:
        args.append(float(accuracy))
    call(name, src.device, *args, src, dst)
    return dst


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


# ---- rays level: caller-supplied rays ---------------------------------------------------------------------------------------

def project_rays(vol, rays, cone, H, W, dVoxel, accuracy=0.5, out=None, projection_type="interpolated"):
    """Line integrals [V,H,W] (GPU, float32) of ``vol`` [nx,ny,nz] (GPU) along caller-supplied rays: ``rays`` [V,12]
    {a, p00, pu, pv} in voxel-index coordinates (include/r2hip.h), ``cone`` the beam (True: from the source a through the
    pixel points; False: through the pixel points along a), ``dVoxel`` the three voxel sizes that scale index lengths to
    world lengths.  No host synchronisation; ``out`` may be a preallocated contiguous float32 GPU tensor [V,H,W]."""
    _check_operand(vol, "vol", "a 3D array [nx,ny,nz]", projection_type)
    check_accuracy(accuracy, projection_type)
    rays = device_rays(rays, vol.device)
    H, W = int(H), int(W)
    out = _output(out, (rays.shape[0], H, W), vol.device, "[%d,%d,%d]" % (rays.shape[0], H, W))
    v32 = f32c(vol)
    return _launch("project", projection_type, rays, cone, H, W, v32.shape, _voxel_sizes(dVoxel), accuracy, v32, out)


def backproject_rays(projs, rays, cone, nVoxel, dVoxel, accuracy=0.5, out=None, projection_type="interpolated"):
    """The exact transpose of ``project_rays``: vol [nx,ny,nz] (GPU, float32) = A^T projs for projections [V,H,W] (GPU) of
    the same ``rays``.  The volume's shape is ``nVoxel``, or that of ``out`` (a contiguous float32 GPU tensor, overwritten)
    where ``nVoxel`` is None.  No host synchronisation."""
    _check_operand(projs, "projs", "[V,H,W]", projection_type)
    check_accuracy(accuracy, projection_type)
    rays = device_rays(rays, projs.device)
    V, H, W = projs.shape
    if rays.shape[0] != V:
        raise ValueError("%d projections for %d views' rays" % (V, rays.shape[0]))
    out = _volume_output(out, nVoxel, projs.device)
    return _launch("backproject", projection_type, rays, cone, H, W, out.shape, _voxel_sizes(dVoxel), accuracy, f32c(projs),
                   out)


# ---- views level: the rasterizer's cameras --------------------------------------------------------------------------------------

def project_views(vol, views, sVoxel, center, accuracy=0.5, out=None, projection_type="interpolated"):
    """Line integrals of ``vol`` [nx,ny,nz] (GPU, the query() / voxelizer layout) along the rays of every pixel of ``views``
    (``scene.View`` list, one detector size): a GPU tensor [V,H,W] in scene units.  ``sVoxel`` / ``center``: the volume's
    extent and centre in the views' (scene) units.  No host synchronisation; ``out`` may be a preallocated [V,H,W] float32
    contiguous GPU tensor.  ``projection_type``: "interpolated" or "siddon" (which ignores ``accuracy``)."""
    _check_operand(vol, "vol", "a 3D array [nx,ny,nz]", projection_type)
    views, H, W = check_views(views)
    _check_extent(sVoxel, center)
    n = tuple(vol.shape)
    return project_rays(vol, ray_params(views, sVoxel, center, n), views[0].mode == 1, H, W,
                        [float(s) / m for s, m in zip(sVoxel, n)], accuracy, out, projection_type)


def backproject_views(projs, views, sVoxel, center, accuracy=0.5, out=None, nVoxel=None, projection_type="interpolated"):
    """The exact transpose of ``project_views``: vol [nx,ny,nz] (GPU) = A^T projs for projections [V,H,W] (GPU, float32) of
    ``views`` (scene units).  The volume's shape comes from ``out`` (a contiguous float32 GPU tensor, overwritten) or
    ``nVoxel``.  No host synchronisation.  ``projection_type`` as in ``project_views``."""
    _check_operand(projs, "projs", "[V,H,W]", projection_type)
    views, H, W = check_views(views)
    if tuple(projs.shape) != (len(views), H, W):
        raise ValueError("projs shape %s differs from the views' [%d,%d,%d]" % (tuple(projs.shape), len(views), H, W))
    _check_extent(sVoxel, center)
    out = _volume_output(out, nVoxel, projs.device)
    n = tuple(out.shape)
    return backproject_rays(projs, ray_params(views, sVoxel, center, n), views[0].mode == 1, None,
                            [float(s) / m for s, m in zip(sVoxel, n)], accuracy, out, projection_type)


# ---- config level: the raw scanner config and its length units -------------------------------------------------------------------

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
    check_accuracy(acc, projection_type)
    if not v.is_cuda:
        v = v.to(device)
    scale = 2.0 / max(cfg["sVoxel"])   # make_view works in the normalised scene (dataset_readers.py:62-76)
    H, W = (int(n) for n in cfg["nDetector"])
    views = [S.make_view(float(a), (H, W), cfg) for a in np.asarray(angles, dtype=np.float64).reshape(-1)]
    out = project_views(v, views, [s * scale for s in cfg["sVoxel"]], [o * scale for o in cfg["offOrigin"]], acc,
                        projection_type=projection_type)
    return out.mul_(1.0 / scale)


class Operator:
    """A = ``project(., angles, cfg)`` and its transpose on one device, with the rays computed once: ``A(x, v0, v1)`` projects
    views v0..v1-1, ``At(p, v0, v1)`` back-projects them.  ``projection_type``: "interpolated" or "siddon" (which ignores
    ``accuracy``), the model of both."""

    def __init__(self, angles, cfg, accuracy=None, device="cuda", projection_type="interpolated"):
        self.projection_type = check_projection_type(projection_type)
        self.cfg = cfg
        acc = cfg.get("accuracy", 0.5) if accuracy is None else accuracy
        check_accuracy(acc, projection_type)
        self.accuracy = float(acc)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.R2HipError("the reconstructions run on the MI355X kernels: device must be a GPU, got %s" % device)
        self.nVoxel = tuple(int(n) for n in cfg["nVoxel"])
        self.H, self.W = (int(n) for n in cfg["nDetector"])
        scale = 2.0 / max(cfg["sVoxel"])   # make_view works in the normalised scene (dataset_readers.py:62-76)
        self.inv_scale = 1.0 / scale
        ang = np.asarray(angles, dtype=np.float64).reshape(-1)
        if ang.size == 0:
            raise ValueError("no angles")
        self.V = int(ang.size)
        views = [S.make_view(float(a), (self.H, self.W), cfg) for a in ang]
        self.cone = views[0].mode == 1
        sV = [s * scale for s in cfg["sVoxel"]]
        self.dVoxel = [s / n for s, n in zip(sV, self.nVoxel)]
        self.rays = device_rays(ray_params(views, sV, [o * scale for o in cfg["offOrigin"]], self.nVoxel), self.device)

    def A(self, x, v0=0, v1=None, out=None):
        v1 = self.V if v1 is None else v1
        if tuple(x.shape) != self.nVoxel:
            raise ValueError("volume shape %s differs from the config's nVoxel %s" % (tuple(x.shape), self.nVoxel))
        out = project_rays(x, self.rays[v0:v1], self.cone, self.H, self.W, self.dVoxel, self.accuracy, out,
                           self.projection_type)
        return out.mul_(self.inv_scale)

    def At(self, p, v0=0, v1=None, out=None):
        v1 = self.V if v1 is None else v1
        if tuple(p.shape) != (v1 - v0, self.H, self.W):
            raise ValueError("projections %s are not views %d..%d of [%d,%d]" % (tuple(p.shape), v0, v1 - 1, self.H, self.W))
        out = backproject_rays(p, self.rays[v0:v1], self.cone, self.nVoxel, self.dVoxel, self.accuracy, out,
                               self.projection_type)
        return out.mul_(self.inv_scale)


def _projections(projs, op):
    p = projs if isinstance(projs, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(projs))
    if p.dim() != 3 or tuple(p.shape) != (op.V, op.H, op.W):
        raise ValueError("projections must be [%d,%d,%d] (one per angle, the config's nDetector), got %s"
                         % (op.V, op.H, op.W, tuple(p.shape)))
    if p.is_floating_point() is False:
        raise ValueError("projections must be floating point, got %s" % (p.dtype,))
    if not p.is_cuda:
        p = p.to(_F32).contiguous().pin_memory()
    return p.to(device=op.device, dtype=_F32, non_blocking=True).contiguous()


def backproject(projs, angles, scanner_cfg, accuracy=None, device="cuda", projection_type="interpolated"):
    """The transpose of ``project``: vol [nx,ny,nz] (GPU tensor) = A^T projs for projections [V,H,W] at ``angles`` with the raw
    scanner config, including ``project``'s 1 / scale."""
    op = Operator(angles, scanner_cfg, accuracy, device, projection_type)
    return op.At(_projections(projs, op))
