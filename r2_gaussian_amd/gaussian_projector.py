"""Exact projection of the Gaussian model: the line integrals of the cloud itself along the rays of every detector pixel, on
the kernels of csrc/gaussian_project.hip, csrc/gaussian_project_bwd.hip and csrc/gaussian_project_rays_bwd.hip
(``r2_project_gaussians`` and its two backwards; include/r2hip.h states the contract).

The splatting rasterizer is the reference's approximation of this image: affine at each Gaussian's centre in cone beam, cut
at a square of ceil(3 sigma_max) pixels, culled at the near plane.  Here every (Gaussian, ray) pair is the closed-form integral
over the whole line; in cone beam a pair whose closest approach lies at or behind the source contributes 0, a pair is only
skipped when its exponent q exceeds 32 (below exp(-16) of the Gaussian's peak), and nothing is culled at a near plane.  The
rays are the [V,12] parameters of the volume projectors (projector.py), in world coordinates, so a detector the rasterizer's
camera cannot describe (shifted, tilted) can be projected with ``project_gaussians_rays``.
"""
import torch

from . import _lib
from . import projector
from ._C import _on_device, _stream

_F32 = torch.float32


def world_ray_params(views):
    """[V,12] float32 ray parameters {a, p00, pu, pv} of ``views`` (``scene.View`` list) in world coordinates: what
    ``projector.ray_params`` gives for a unit voxel grid whose index coordinates are the world's."""
    return projector.ray_params(views, (1.0, 1.0, 1.0), (0.0, 0.0, 0.0), (1, 1, 1))


def _f32c(t):
    return t if t.dtype == _F32 and t.is_contiguous() else t.to(_F32).contiguous()


class _ProjectGaussians(torch.autograd.Function):
    @staticmethod
    def forward(ctx, xyz, density, scaling, rotation, rays, cone, H, W, scale_modifier, out):
        V, P = rays.shape[0], xyz.shape[0]
        x, d, s, r = _f32c(xyz.detach()), _f32c(density.detach()), _f32c(scaling.detach()), _f32c(rotation.detach())
        rays = rays.detach()
        with _on_device(x.device):
            rc = _lib.lib().r2_project_gaussians(V, H, W, rays.data_ptr(), cone, P, x.data_ptr(), d.data_ptr(), s.data_ptr(),
                                                 float(scale_modifier), r.data_ptr(), out.data_ptr(), _stream(x.device))
        _lib.check(rc, "r2_project_gaussians")
        ctx.save_for_backward(x, d, s, r, rays)
        ctx.args = (cone, H, W, float(scale_modifier))
        ctx.mark_dirty(out)
        return out

    @staticmethod
    def backward(ctx, G):
        x, d, s, r, rays = ctx.saved_tensors
        cone, H, W, mod = ctx.args
        V, P = rays.shape[0], x.shape[0]
        G = _f32c(G)
        L = _lib.lib()
        gx = gd = gs = gr = grays = None
        if any(ctx.needs_input_grad[:4]):
            gx, gd, gs, gr = torch.empty_like(x), torch.empty_like(d), torch.empty_like(s), torch.empty_like(r)
            with _on_device(x.device):
                rc = L.r2_project_gaussians_backward(V, H, W, rays.data_ptr(), cone, P, x.data_ptr(), d.data_ptr(), s.data_ptr(),
                                                     mod, r.data_ptr(), G.data_ptr(), gx.data_ptr(), gd.data_ptr(), gs.data_ptr(),
                                                     gr.data_ptr(), _stream(x.device))
            _lib.check(rc, "r2_project_gaussians_backward")
        if ctx.needs_input_grad[4]:
            grays = torch.empty_like(rays)
            ws = torch.empty((max(int(L.r2_project_gaussians_rays_backward_workspace_bytes(V, H, W)), 1),), dtype=torch.uint8,
                             device=x.device)
            with _on_device(x.device):
                rc = L.r2_project_gaussians_rays_backward(V, H, W, rays.data_ptr(), cone, P, x.data_ptr(), d.data_ptr(),
                                                          s.data_ptr(), mod, r.data_ptr(), G.data_ptr(), grays.data_ptr(),
                                                          ws.data_ptr(), ws.numel(), _stream(x.device))
            _lib.check(rc, "r2_project_gaussians_rays_backward")
        return gx, gd, gs, gr, grays, None, None, None, None, None


def project_gaussians_rays(rays, cone, H, W, xyz, density, scaling, rotation, scale_modifier=1.0, out=None):
    """Exact projections [V,H,W] (GPU, float32) of the cloud ``xyz`` [P,3], ``density`` [P,1] or [P], ``scaling`` [P,3],
    ``rotation`` [P,4] (activated values; the quaternion is used as it comes) along caller-supplied rays: ``rays`` [V,12]
    {a, p00, pu, pv} in world coordinates (include/r2hip.h), ``cone`` the beam (True: from the source a through the pixel
    points; False: through the pixel points along a).  Differentiable in the four parameter tensors, and in ``rays`` when they
    require grad (``r2_project_gaussians_rays_backward``, launched only then): a ``rays`` tensor on the device or on the host,
    of any float dtype, receives its gradient where and as it is.  No host synchronisation (host rays that require grad are
    copied synchronously); ``out`` may be a preallocated contiguous float32 GPU tensor [V,H,W]."""
    rays = torch.as_tensor(rays)
    if rays.dim() != 2 or rays.shape[1] != 12 or rays.shape[0] < 1:
        raise ValueError("rays must be [V,12] with V >= 1, got shape %s" % (tuple(rays.shape),))
    H, W = int(H), int(W)
    if H < 1 or W < 1:
        raise ValueError("the detector must have at least one pixel, got %d x %d" % (H, W))
    for name, t, cols in (("xyz", xyz, 3), ("scaling", scaling, 3), ("rotation", rotation, 4)):
        if not isinstance(t, torch.Tensor) or t.dim() != 2 or t.shape[1] != cols:
            raise ValueError("%s must be a tensor [P,%d], got %s" % (name, cols, tuple(getattr(t, "shape", ()))))
    P = xyz.shape[0]
    if not isinstance(density, torch.Tensor) or tuple(density.shape) not in ((P, 1), (P,)):
        raise ValueError("density must be a tensor [P,1] or [P] with P = %d, got %s" % (P, tuple(getattr(density, "shape", ()))))
    if scaling.shape[0] != P or rotation.shape[0] != P:
        raise ValueError("xyz, scaling and rotation differ in P: %d, %d, %d" % (P, scaling.shape[0], rotation.shape[0]))
    for name, t in (("xyz", xyz), ("density", density), ("scaling", scaling), ("rotation", rotation)):
        if not t.is_cuda:
            raise ValueError("%s must be a GPU tensor: the exact projector has no CPU fallback" % name)
        if t.device != xyz.device:
            raise ValueError("%s is on %s, xyz on %s" % (name, t.device, xyz.device))
    V = rays.shape[0]
    if out is not None and (not isinstance(out, torch.Tensor) or out.dtype != _F32 or not out.is_cuda or not out.is_contiguous()
                            or tuple(out.shape) != (V, H, W) or out.device != xyz.device):
        raise ValueError("out must be a contiguous float32 tensor [%d,%d,%d] on %s" % (V, H, W, xyz.device))
    if rays.requires_grad:   # differentiable torch ops carry the gradient back to the caller's tensor, device and dtype
        rays = rays.to(device=xyz.device, dtype=_F32).contiguous()
    else:
        rays = projector.device_rays(rays, xyz.device)
    if out is None:
        out = torch.empty((V, H, W), dtype=_F32, device=xyz.device)
    return _ProjectGaussians.apply(xyz, density, scaling, rotation, rays, int(bool(cone)), H, W, float(scale_modifier), out)


def project_gaussians(views, xyz, density, scaling, rotation, scale_modifier=1.0, out=None):
    """Exact projections [V,H,W] of the cloud on ``views`` (``scene.View`` list: one detector size, one beam mode), registered
    to the rasterizer's image of the same view.  See ``project_gaussians_rays``."""
    views, H, W = projector.check_views(views)
    return project_gaussians_rays(torch.from_numpy(world_ray_params(views)), views[0].mode == 1, H, W, xyz, density, scaling,
                                  rotation, scale_modifier, out)
