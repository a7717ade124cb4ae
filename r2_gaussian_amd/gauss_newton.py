"""Gauss-Newton on the exact projector: the normal-equations product ``J^T W J t`` and a Levenberg-Marquardt fit of the cloud
that solves its steps by conjugate gradients, on the kernels of csrc/gaussian_tangent.hip (``r2_project_gaussians_jvp``: J t),
csrc/gaussian_project_bwd.hip (``r2_project_gaussians_backward``: J^T g) and csrc/gaussian_fisher.hip
(``r2_project_gaussians_fisher``: diag J^T W J, the Jacobi preconditioner and Marquardt's scaling).

The fit of a cloud to measured projections is a least-squares problem; with J the Jacobian of the exact image in the cloud's
parameters, r the residual and F = diag(J^T W J), a step solves

    (J^T W J + lambda diag F) delta = -J^T W r

without ever forming J: every CG iteration is one JVP launch and one backward launch.

    cloud, history = refine_cloud(views, projs, cloud, steps=3, cg_iters=3)

``geometry.refine_geometry_lm`` is the same method for the scan geometry, where J is small enough to be formed.
"""
import torch

from . import projector
from ._boundary import call
from .gaussian_projector import (check_projection_arguments, plan_projection_rays, project_gaussians_rays, project_gaussians_rays_jvp,
                                 world_ray_params)
from .uncertainty import CloudTuple, _check_group_tuple, _cloud, fisher_diagonal_rays

_F32, _F64 = torch.float32, torch.float64

# The default of ``max_log_step``: a step in log density or log scale is clipped to +- this, so no density and no scale changes
# by more than a factor e in one step.  A Gaussian the views barely see has a tiny F, Jacobi's 1 / F makes its step huge, and
# exp of an unclipped step underflows to 0 in float32: the Gaussian would be deleted for good (a scale of 0 contributes nothing
# and has no gradient).
MAX_LOG_STEP = 1.0


@torch.no_grad()
def _backward(rays, cone, H, W, cloud, G, scale_modifier):
    """J^T G as a CloudTuple: ``r2_project_gaussians_backward`` on detached tensors, outside autograd."""
    V, dev = rays.shape[0], G.device
    x, d, s, r = _cloud(*cloud)
    P = x.shape[0]
    out = CloudTuple(torch.empty((P, 3), dtype=_F32, device=dev), torch.empty((P, 1), dtype=_F32, device=dev),
                     torch.empty((P, 3), dtype=_F32, device=dev), torch.empty((P, 4), dtype=_F32, device=dev))
    call("r2_project_gaussians_backward", dev, V, H, W, rays, int(bool(cone)), P, x, d, s, float(scale_modifier), r, G, *out)
    return out


def _check_weights(weights, V, H, W, dev):
    if weights is None:
        return None
    if not isinstance(weights, torch.Tensor) or tuple(weights.shape) != (V, H, W) or weights.device != dev:
        raise ValueError("weights must be a tensor [%d,%d,%d] on %s, got %s" % (V, H, W, dev, tuple(getattr(weights, "shape", ()))))
    return weights.detach().to(_F32)


@torch.no_grad()
def normal_matvec(rays, cone, H, W, cloud, tangents, weights=None, damping=0.0, fisher=None, scale_modifier=1.0, planned=False):
    """``J^T W J t + damping * F * t`` as a ``CloudTuple``: the normal-equations operator of the weighted least-squares fit of
    ``project_gaussians_rays`` on (``rays``, ``cone``, ``H``, ``W``, ``cloud``), applied to ``tangents`` (a 4-tuple shaped like
    the cloud).  One ``r2_project_gaussians_jvp`` launch and one ``r2_project_gaussians_backward`` launch; J is never formed.
    ``weights`` [V,H,W] (GPU, >= 0; None: 1).  ``fisher``: F, a 4-tuple (``uncertainty.fisher_diagonal_rays`` with the same
    weights); it is read only when ``damping`` is not 0, and computed when it is needed and not given.  float32; no host
    synchronisation.  ``planned``: build a ``ProjectionPlan`` of (rays, cloud) and let the JVP walk its lists -- the same bits,
    and ONE host read for the plan (``gaussian_projector.plan_projection_rays``); a single product does not repay the build,
    the solvers below share one plan among a cloud's launches."""
    cloud = tuple(cloud)
    rays, H, W = check_projection_arguments(rays, H, W, *cloud)
    V, P, dev = rays.shape[0], cloud[0].shape[0], cloud[0].device
    weights = _check_weights(weights, V, H, W, dev)
    t = _check_group_tuple(tangents, P, dev, "tangents")
    rays = projector.device_rays(rays.detach(), dev)
    plan = plan_projection_rays(rays, cone, H, W, *cloud, scale_modifier=scale_modifier) if planned else None
    jt = project_gaussians_rays_jvp(rays, cone, H, W, *cloud, tangents=t, scale_modifier=scale_modifier, plan=plan)
    if weights is not None:
        jt = jt * weights
    out = _backward(rays, cone, H, W, cloud, jt, scale_modifier)
    if damping:
        if fisher is None:
            fisher = fisher_diagonal_rays(rays, cone, H, W, *cloud, weights=weights, scale_modifier=scale_modifier)
        F = _check_group_tuple(fisher, P, dev, "fisher")
        out = CloudTuple(*(o + float(damping) * f.reshape(o.shape) * v.reshape(o.shape) for o, f, v in zip(out, F, t)))
    return out


def _flat(groups):
    """A 4-tuple shaped like the cloud -> [P,11] float32."""
    return torch.cat([g.reshape(g.shape[0], -1) for g in groups], 1)


def _split(flat):
    """[P,11] -> CloudTuple of contiguous tensors."""
    return CloudTuple(flat[:, 0:3].contiguous(), flat[:, 3:4].contiguous(), flat[:, 4:7].contiguous(), flat[:, 7:11].contiguous())


def _log_factors(cloud, log_density, log_scaling):
    """[P,11] float32: what a tangent in the solver's variables is multiplied by to become one in the kernels' parameters."""
    x, d, s, r = _cloud(*cloud)
    return torch.cat([torch.ones_like(x), d.reshape(-1, 1) if log_density else torch.ones_like(d.reshape(-1, 1)),
                      s if log_scaling else torch.ones_like(s), torch.ones_like(r)], 1)


def _loss(rays, cone, H, W, cloud, target, weights, scale_modifier, plan=None):
    """-> (residual [V,H,W] float32, the mean weighted squared error: a float64 scalar on the device)."""
    res = project_gaussians_rays(rays, cone, H, W, *cloud, scale_modifier=scale_modifier, plan=plan) - target
    sq = res.to(_F64) ** 2
    return res, (sq if weights is None else sq * weights.to(_F64)).mean()


def _check_solver_arguments(cg_iters, damping, max_log_step):
    if int(cg_iters) < 1:
        raise ValueError("cg_iters must be at least 1, got %r" % (cg_iters,))
    if not float(damping) >= 0:
        raise ValueError("damping must be >= 0, got %r" % (damping,))
    if not float(max_log_step) > 0:
        raise ValueError("max_log_step must be positive, got %r" % (max_log_step,))


@torch.no_grad()
def _linearise(rays, cone, H, W, cloud, res, weights, log_density, log_scaling, scale_modifier):
    """What a step's system is made of at ``cloud`` with the residual ``res``, and what stays the same while the cloud does:
    -> (f: the log factors, F: diag(J^T W J) in the solver's variables, b = -J^T W r), each [P,11] float32.  One Fisher launch
    and one backward launch."""
    f = _log_factors(cloud, log_density, log_scaling)
    F = _flat(fisher_diagonal_rays(rays, cone, H, W, *cloud, weights=weights, scale_modifier=scale_modifier)) * (f * f)
    b = -(_flat(_backward(rays, cone, H, W, cloud, res if weights is None else res * weights, scale_modifier)) * f)
    return f, F, b


@torch.no_grad()
def _solve_and_move(rays, cone, H, W, cloud, lin, cg_iters, lam, weights, log_density, log_scaling, scale_modifier, max_log_step,
                    plan=None):
    """``cg_iters`` CG iterations on (J^T W J + lam diag F) delta = b from delta = 0, and the cloud moved by delta; ``plan``:
    the ``ProjectionPlan`` of (rays, cloud) every JVP walks, or None."""
    f, F, b = lin

    def matvec(t):
        jt = project_gaussians_rays_jvp(rays, cone, H, W, *cloud, tangents=_split(t * f), scale_modifier=scale_modifier, plan=plan)
        if weights is not None:
            jt = jt * weights
        return _flat(_backward(rays, cone, H, W, cloud, jt, scale_modifier)) * f + lam * F * t

    dot = lambda a, c: (a.to(_F64) * c.to(_F64)).sum()
    M = (1.0 + lam) * F.to(_F64)
    minv = torch.where(M > 0, 1.0 / torch.where(M > 0, M, torch.ones_like(M)), torch.zeros_like(M)).to(_F32)
    zero = torch.zeros((), dtype=_F64, device=b.device)
    x = torch.zeros_like(b)
    r = b.clone()
    z = minv * r
    p = z.clone()
    rz = dot(r, z)
    for _ in range(int(cg_iters)):
        Ap = matvec(p)
        pAp = dot(p, Ap)
        alpha = torch.where(pAp > 0, rz / torch.where(pAp > 0, pAp, torch.ones_like(pAp)), zero).to(_F32)
        x = x + alpha * p
        r = r - alpha * Ap
        z = minv * r
        rz_new = dot(r, z)
        beta = torch.where(rz > 0, rz_new / torch.where(rz > 0, rz, torch.ones_like(rz)), zero).to(_F32)
        p = z + beta * p
        rz = rz_new
    d = _split(x)
    clip = lambda t: t.clamp(-float(max_log_step), float(max_log_step))
    return CloudTuple(cloud.xyz + d.xyz, cloud.density * torch.exp(clip(d.density)) if log_density else cloud.density + d.density,
                      cloud.scaling * torch.exp(clip(d.scaling)) if log_scaling else cloud.scaling + d.scaling,
                      cloud.rotation + d.rotation)


def _kernel_cloud(cloud):
    """Detached contiguous float32 tensors [P,3], [P,1], [P,3], [P,4]."""
    P = cloud[0].shape[0]
    return CloudTuple(*(c.reshape(P, -1) for c in _cloud(*cloud)))


@torch.no_grad()
def gauss_newton_step(rays, cone, H, W, cloud, projs, cg_iters, damping, weights=None, log_density=True, log_scaling=True,
                      scale_modifier=1.0, max_log_step=MAX_LOG_STEP, planned=False):
    """One damped Gauss-Newton step of the weighted least-squares fit of the cloud to ``projs`` [V,H,W] (GPU): solves
    ``(J^T W J + damping diag F) delta = -J^T W r``, r = image - projs, F = diag(J^T W J), by ``cg_iters`` iterations of
    conjugate gradients from delta = 0 -- a fixed count, so nothing waits for the device -- preconditioned by Jacobi,
    1 / ((1 + damping) F) from ``uncertainty.fisher_diagonal_rays`` (0 where F is 0: a Gaussian no ray touches does not move).
    ``log_density`` / ``log_scaling``: the step is taken in log density / log scales, which multiplies tangents and gradients
    by the parameter and F by its square, and the update multiplies by exp(delta) with delta clipped to +- ``max_log_step``:
    density and scales stay positive, in float32 too (``MAX_LOG_STEP`` says why).  The quaternion moves additively and is not
    renormalised (the projector uses it as it comes).
    Launches: one forward, one Fisher, one backward, then one JVP and one backward per CG iteration.  The CG vectors are
    float32, its scalars float64 on the device; an iteration whose curvature is not positive changes nothing.
    ``planned``: one ``ProjectionPlan`` of (rays, cloud) is built first and serves the forward and every JVP of the CG, which
    then walk per-tile lists instead of the whole cloud: the same bits, fewer tests, and ONE host read, of the plan's instance
    count (``gaussian_projector.plan_projection_rays``).  The Fisher and the backward launches are Gaussian-major and unchanged.
    -> (the moved cloud: a ``CloudTuple`` of float32 tensors, the loss BEFORE the step: the mean weighted squared error, a
    float64 scalar on the device)."""
    cloud = tuple(cloud)
    rays, H, W = check_projection_arguments(rays, H, W, *cloud)
    V, dev = rays.shape[0], cloud[0].device
    if not isinstance(projs, torch.Tensor) or tuple(projs.shape) != (V, H, W) or projs.device != dev:
        raise ValueError("projs must be a tensor [%d,%d,%d] on %s, got %s" % (V, H, W, dev, tuple(getattr(projs, "shape", ()))))
    _check_solver_arguments(cg_iters, damping, max_log_step)
    weights = _check_weights(weights, V, H, W, dev)
    rays = projector.device_rays(rays.detach(), dev)
    cloud = _kernel_cloud(cloud)
    plan = plan_projection_rays(rays, cone, H, W, *cloud, scale_modifier=scale_modifier) if planned else None
    res, loss = _loss(rays, cone, H, W, cloud, projs.detach().to(_F32), weights, scale_modifier, plan)
    lin = _linearise(rays, cone, H, W, cloud, res, weights, log_density, log_scaling, scale_modifier)
    return _solve_and_move(rays, cone, H, W, cloud, lin, cg_iters, float(damping), weights, log_density, log_scaling, scale_modifier,
                           max_log_step, plan), loss


def refine_cloud(views, projs, cloud, steps, cg_iters, damping=1e-3, cone=True, weights=None, log_density=True, log_scaling=True,
                 scale_modifier=1.0, callback=None, max_log_step=MAX_LOG_STEP, planned=False):
    """Levenberg-Marquardt fit of the cloud to ``projs`` [V,H,W] (GPU) on the exact projector: ``steps`` steps of
    ``gauss_newton_step``'s solve with the accept / reject rule of ``geometry.refine_geometry_lm`` -- the candidate is taken
    when the mean weighted squared error falls, ``damping`` is divided by 10 then and multiplied by 10 otherwise (the cloud
    stays).  ``views``: a ``scene.View`` list (one detector size, one beam mode), or rays [V,12] {a, p00, pu, pv} in world
    coordinates with ``cone`` the beam.  ``cloud`` = (xyz, density, scaling, rotation), activated GPU tensors; the number of
    Gaussians does not change.  Per step: the CG's launches and ONE forward, of the candidate, whose residual serves the
    next step when it is taken; the Fisher diagonal and the right-hand side are computed once per accepted cloud and kept
    across rejected steps.  One host read per step, of the comparison that decides it.
    ``planned``: every cloud that is projected gets a ``ProjectionPlan`` -- the start, then each candidate -- which serves its
    forward and, when the candidate is taken, every JVP of the next steps' CG until another candidate is; the same bits, and
    one more host read per plan (``gaussian_projector.plan_projection_rays``), so two per step.
    -> (the refined cloud: a ``CloudTuple`` of float32 tensors, loss history: a float64 tensor [steps] on the device, the loss
    BEFORE each step).  ``callback(step, loss, cloud)``, when given, runs after every step."""
    if isinstance(views, (list, tuple)) and views and hasattr(views[0], "world_view_transform"):
        views, H, W = projector.check_views(views)
        rays, cone = torch.from_numpy(world_ray_params(views)), views[0].mode == 1
    else:
        rays = torch.as_tensor(views)
    if not isinstance(projs, torch.Tensor) or projs.dim() != 3 or not projs.is_cuda:
        raise ValueError("projs must be a GPU tensor [V,H,W]")
    H, W = projs.shape[1], projs.shape[2]
    cloud = tuple(t.detach() for t in cloud)
    rays, H, W = check_projection_arguments(rays, H, W, *cloud)
    if tuple(projs.shape) != (rays.shape[0], H, W) or projs.device != cloud[0].device:
        raise ValueError("projs must be [%d,%d,%d] on %s, got %s on %s" % (rays.shape[0], H, W, cloud[0].device, tuple(projs.shape),
                                                                          projs.device))
    _check_solver_arguments(cg_iters, damping, max_log_step)
    rays = projector.device_rays(rays.detach(), projs.device)
    weights = _check_weights(weights, rays.shape[0], H, W, projs.device)
    target = projs.detach().to(_F32)
    cloud = _kernel_cloud(cloud)
    lam = float(damping)
    history = torch.zeros((int(steps),), dtype=_F64, device=projs.device)
    make_plan = lambda c: plan_projection_rays(rays, cone, H, W, *c, scale_modifier=scale_modifier) if planned else None
    plan = make_plan(cloud)
    res, loss = _loss(rays, cone, H, W, cloud, target, weights, scale_modifier, plan)
    lin = None
    for it in range(int(steps)):
        history[it] = loss
        if lin is None:   # a new cloud: its Fisher diagonal and right-hand side
            lin = _linearise(rays, cone, H, W, cloud, res, weights, log_density, log_scaling, scale_modifier)
        cand = _solve_and_move(rays, cone, H, W, cloud, lin, cg_iters, lam, weights, log_density, log_scaling, scale_modifier,
                               max_log_step, plan)
        plan_c = make_plan(cand)
        res_c, loss_c = _loss(rays, cone, H, W, cand, target, weights, scale_modifier, plan_c)
        if bool(loss_c < loss):   # the one host read of the step
            cloud, res, loss, lin, lam, plan = cand, res_c, loss_c, None, lam / 10.0, plan_c
        else:
            lam = lam * 10.0
        if callback is not None:
            callback(it, history[it], cloud)
    return cloud, history
