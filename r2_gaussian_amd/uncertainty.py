"""How far the measured views pin the Gaussian model down, and where the volume is a guess: the diagonal of the Fisher
information of the exact projector, and the predictive variances that follow from it, on the kernels of
csrc/gaussian_fisher.hip and csrc/gaussian_variance.hip (``r2_project_gaussians_fisher``, ``r2_query_gaussians_variance``,
``r2_project_gaussians_variance``; include/r2hip.h states the contract).

The exact image is a plain sum over the Gaussians, so the derivative of one pixel with respect to one parameter of one
Gaussian is one pair's number, and the sum of its weighted squares over the pixels is the diagonal of ``J^T W J``: the Fisher
information of the parameters under independent pixel noise of variance ``1 / w``, the Gauss-Newton diagonal of the weighted
least-squares fit.  Autograd yields ``J^T g``, never the squares.

    F = fisher_diagonal(views, xyz, density, scaling, rotation, weights)       # [P,3], [P,1], [P,3], [P,4]
    var = parameter_variance(F, prior_precision)                               # Laplace: 1 / (F + lambda)
    field_variance(points, ..., var)      projection_variance(views, ..., var)    view_information(candidates, ..., var)

Everything here is diagonal: correlations between the parameters of a Gaussian and between Gaussians are ignored.  It is a
Laplace approximation in the given parametrisation (activated means, densities, scales, the quaternion as it comes), not a
posterior.  The exact projector stands for the model, as it does in ``train.py --eval_exact``.
"""
import collections

import numpy as np
import torch

from . import projector
from ._boundary import _F32, NAMES, WIDTHS, call, cloud, f32c, require_gpu
from .field import _check_cloud, inverse_permutation, morton_order
from .gaussian_projector import _call_planned, _checked_plan, check_projection_arguments, world_ray_params

CloudTuple = collections.namedtuple("CloudTuple", NAMES)
CloudTuple.__doc__ = "One float32 tensor per parameter group, in the shapes of the cloud: [P,3], [P,1], [P,3], [P,4]."


def _cloud(xyz, density, scaling, rotation):
    """Detached contiguous float32 copies (or the tensors themselves) for the kernels; density as [P]."""
    x, d, s, r = cloud(xyz, density, scaling, rotation)
    return x, d.reshape(-1), s, r


def _check_group_tuple(t, P, device, name):
    """A 4-tuple (xyz [P,3], density [P,1] or [P], scaling [P,3], rotation [P,4]) on ``device`` -> four contiguous float32."""
    if not isinstance(t, (tuple, list)) or len(t) != 4:
        raise ValueError("%s must be a 4-tuple (xyz, density, scaling, rotation), got %r" % (name, type(t).__name__))
    out = []
    for (g, cols), a in zip(WIDTHS.items(), t):
        ok = isinstance(a, torch.Tensor) and (tuple(a.shape) == (P, cols) or (cols == 1 and tuple(a.shape) == (P,)))
        if not ok:
            raise ValueError("%s.%s must be a tensor [%d,%d], got %s" % (name, g, P, cols, tuple(getattr(a, "shape", ()))))
        if a.device != device:
            raise ValueError("%s.%s is on %s, xyz on %s" % (name, g, a.device, device))
        out.append(f32c(a.detach()).reshape(-1) if cols == 1 else f32c(a.detach()))
    return out


@torch.no_grad()
def fisher_diagonal_rays(rays, cone, H, W, xyz, density, scaling, rotation, weights=None, scale_modifier=1.0):
    """The diagonal of ``J^T W J`` of ``project_gaussians_rays`` on the same arguments: for every parameter of every Gaussian
    the sum over the pixels of all views of ``w (d image / d parameter)^2``.  ``weights`` [V,H,W] (GPU, >= 0; None: 1) are
    the inverse variances of the pixels (``noise_weights``).  -> ``CloudTuple(xyz [P,3], density [P,1], scaling [P,3],
    rotation [P,4])``, float32.  The parameters are the projector's gradient's: the scales as given (the ``scale_modifier``
    factor included), the quaternion as it comes.  Not differentiable.  One launch, no host synchronisation, the same bits on
    every call; a Gaussian no ray touches gets exact zeros.  Cost: that of the projector's parameter backward."""
    rays, H, W = check_projection_arguments(rays, H, W, xyz, density, scaling, rotation)
    V, P, dev = rays.shape[0], xyz.shape[0], xyz.device
    if weights is not None:
        if not isinstance(weights, torch.Tensor) or tuple(weights.shape) != (V, H, W) or weights.device != dev:
            raise ValueError("weights must be a tensor [%d,%d,%d] on %s, got %s" % (V, H, W, dev, tuple(getattr(weights, "shape", ()))))
        weights = f32c(weights.detach())
    rays = projector.device_rays(rays.detach(), dev)
    x, d, s, r = _cloud(xyz, density, scaling, rotation)
    F = CloudTuple(torch.empty((P, 3), dtype=_F32, device=dev), torch.empty((P, 1), dtype=_F32, device=dev),
                   torch.empty((P, 3), dtype=_F32, device=dev), torch.empty((P, 4), dtype=_F32, device=dev))
    call("r2_project_gaussians_fisher", dev, V, H, W, rays, int(bool(cone)), P, x, d, s, float(scale_modifier), r, weights, *F)
    return F


def fisher_diagonal(views, xyz, density, scaling, rotation, weights=None, scale_modifier=1.0):
    """``fisher_diagonal_rays`` on ``views`` (``scene.View`` list: one detector size, one beam mode), as ``project_gaussians``
    is to ``project_gaussians_rays``."""
    views, H, W = projector.check_views(views)
    return fisher_diagonal_rays(torch.from_numpy(world_ray_params(views)), views[0].mode == 1, H, W, xyz, density, scaling,
                                rotation, weights, scale_modifier)


def parameter_variance(fisher, prior_precision):
    """The Laplace variance of every parameter, ``1 / (F + lambda)`` per group: ``fisher`` a 4-tuple of tensors (what
    ``fisher_diagonal`` returns), ``prior_precision`` a positive number or one per group (xyz, density, scaling, rotation).
    lambda <= 0 raises: a Gaussian no view sees has F = 0, and without a prior its variance is not finite."""
    if not isinstance(fisher, (tuple, list)) or len(fisher) != 4 or not all(isinstance(f, torch.Tensor) for f in fisher):
        raise ValueError("fisher must be a 4-tuple of tensors (xyz, density, scaling, rotation)")
    lam = tuple(prior_precision) if isinstance(prior_precision, (tuple, list)) else (prior_precision,) * 4
    if len(lam) != 4:
        raise ValueError("prior_precision must be one number or four (xyz, density, scaling, rotation), got %d" % len(lam))
    lam = tuple(float(v) for v in lam)
    if not all(v > 0 and v < float("inf") for v in lam):
        raise ValueError("prior_precision must be positive and finite, got %r" % (lam,))
    return CloudTuple(*(1.0 / (f + v) for f, v in zip(fisher, lam)))


@torch.no_grad()
def field_variance(points, xyz, density, scaling, rotation, variance, scale_modifier=1.0, sort=False):
    """The predictive variance of the density field at ``points`` [..., 3] -> [...] (GPU, float32) under independent parameter
    variances ``variance`` (a 4-tuple in the cloud's shapes, >= 0; ``parameter_variance``): the sum over the pairs
    ``field.query_points`` sums of ``sum_t variance_t (d term / d parameter_t)^2``.  ``sort`` as in ``query_points``: a Morton
    gather and scatter that changes the cost alone -- a point's value depends on the cloud and the point, bit for bit.  Not
    differentiable.  No host synchronisation."""
    if not isinstance(points, torch.Tensor) or points.dim() < 1 or points.shape[-1] != 3:
        raise ValueError("points must be a tensor [..., 3], got %s" % (tuple(getattr(points, "shape", ())),))
    require_gpu(points, "points")
    _check_cloud(xyz, density, scaling, rotation)
    dev, P = xyz.device, xyz.shape[0]
    if points.device != dev:
        raise ValueError("points are on %s, xyz on %s" % (points.device, dev))
    vx, vd, vs, vr = _check_group_tuple(variance, P, dev, "variance")
    pts = f32c(points.detach().reshape(-1, 3))
    N = pts.shape[0]
    if N >= (1 << 31):
        raise ValueError("fewer than 2^31 points, got %d" % N)
    inv = None
    if sort:
        perm = morton_order(pts)
        pts, inv = pts[perm].contiguous(), inverse_permutation(perm)
    x, d, s, r = _cloud(xyz, density, scaling, rotation)
    out = torch.empty((N,), dtype=_F32, device=dev)
    call("r2_query_gaussians_variance", dev, N, pts, P, x, d, s, float(scale_modifier), r, vx, vd, vs, vr, out)
    if inv is not None:
        out = out[inv]
    return out.reshape(points.shape[:-1])


@torch.no_grad()
def projection_variance_rays(rays, cone, H, W, xyz, density, scaling, rotation, variance, scale_modifier=1.0, plan=None):
    """The predictive variance [V,H,W] (GPU, float32) of every pixel of ``project_gaussians_rays`` on the same arguments, under
    independent parameter variances ``variance``.  Not differentiable.  No host synchronisation.  ``plan``: a
    ``gaussian_projector.ProjectionPlan`` built from these very tensors; the launch then walks its lists
    (``r2_project_gaussians_variance_planned``) and gives the same bits."""
    rays, H, W = check_projection_arguments(rays, H, W, xyz, density, scaling, rotation)
    plan = _checked_plan(plan, rays, cone, H, W, xyz, density, scaling, rotation, scale_modifier)
    V, P, dev = rays.shape[0], xyz.shape[0], xyz.device
    vx, vd, vs, vr = _check_group_tuple(variance, P, dev, "variance")
    rays = projector.device_rays(rays.detach(), dev)
    x, d, s, r = _cloud(xyz, density, scaling, rotation)
    out = torch.empty((V, H, W), dtype=_F32, device=dev)
    _call_planned("r2_project_gaussians_variance", plan, dev, V, H, W, rays, int(bool(cone)), P, x, d, s, float(scale_modifier), r,
                  vx, vd, vs, vr, out)
    return out


def projection_variance(views, xyz, density, scaling, rotation, variance, scale_modifier=1.0, plan=None):
    """``projection_variance_rays`` on ``views`` (``scene.View`` list) -> [V,H,W]; ``plan``: from
    ``gaussian_projector.plan_projection``."""
    from .gaussian_projector import _view_rays
    views, H, W = projector.check_views(views)
    return projection_variance_rays(_view_rays(views, plan), views[0].mode == 1, H, W, xyz, density, scaling, rotation, variance,
                                    scale_modifier, plan)


def view_information(views, xyz, density, scaling, rotation, variance, weights=None, scale_modifier=1.0):
    """The expected information [V] (float64, on the cloud's device) of each candidate view that has not been measured yet:
    ``sum_it F_view,it variance_it``, F_view the Fisher diagonal of that view alone -- the next-best-view score (the FisherRF
    acquisition function on the diagonal); the view with the largest score is the one the current model is least sure
    about.  ``weights`` [V,H,W] or None: the expected inverse noise variance of the candidates' pixels.  One Fisher launch per
    candidate, reduced in float64."""
    views, H, W = projector.check_views(views)
    P, dev = xyz.shape[0], xyz.device
    rays = torch.from_numpy(world_ray_params(views))
    check_projection_arguments(rays, H, W, xyz, density, scaling, rotation)
    var = [v.to(torch.float64).reshape(P, -1) for v in _check_group_tuple(variance, P, dev, "variance")]
    if weights is not None and (not isinstance(weights, torch.Tensor) or tuple(weights.shape) != (len(views), H, W)):
        raise ValueError("weights must be a tensor [%d,%d,%d], got %s" % (len(views), H, W, tuple(getattr(weights, "shape", ()))))
    scores = []
    for i in range(len(views)):
        F = fisher_diagonal_rays(rays[i:i + 1], views[0].mode == 1, H, W, xyz, density, scaling, rotation,
                                 None if weights is None else weights[i:i + 1], scale_modifier)
        scores.append(sum((f.to(torch.float64) * v).sum() for f, v in zip(F, var)))
    return torch.stack(scores)


def noise_weights(projs, i0, gaussian, m=None):
    """The inverse variance of every pixel of a log-transformed projection stack under ``datagen.add_noise``'s model,
    I = Poisson(i0 exp(-p / m)) + Normal(mu, sigma), p_noisy = -m log(I / i0): to first order
    ``Var(p_noisy) = m^2 Var(I) / Ibar^2`` with ``Ibar = i0 exp(-p / m)`` and ``Var(I) = Ibar + sigma^2``, so
    ``w = Ibar^2 / (m^2 (Ibar + sigma^2))``.  ``projs``: a numpy array or a tensor (the result is of the same kind, float32);
    ``gaussian`` = (mu, sigma); ``m``: the stack's maximum when not given, as in ``add_noise``.  An all-zero stack, which
    ``add_noise`` leaves without noise, gives ones."""
    _mu, sigma = (float(v) for v in gaussian)
    is_tensor = isinstance(projs, torch.Tensor)
    p = projs.detach().to(torch.float64) if is_tensor else torch.from_numpy(np.asarray(projs, dtype=np.float64))
    m = float(p.max()) if m is None and p.numel() else (0.0 if m is None else float(m))
    if not m > 0:
        w = torch.ones_like(p)
    else:
        ibar = float(i0) * torch.exp(-p / m)
        w = ibar * ibar / (m * m * (ibar + sigma * sigma))
    w = w.to(_F32)
    return w if is_tensor else w.numpy()
