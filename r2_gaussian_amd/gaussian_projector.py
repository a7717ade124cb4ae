"""Exact projection of the Gaussian model: the line integrals of the cloud itself along the rays of every detector pixel, on
the kernels of csrc/gaussian_project.hip, csrc/gaussian_project_bwd.hip and csrc/gaussian_project_rays_bwd.hip
(``r2_project_gaussians`` and its two backwards; include/r2hip.h states the contract).

The splatting rasterizer is the reference's approximation of this image: affine at each Gaussian's centre in cone beam, cut
at a square of ceil(3 sigma_max) pixels, culled at the near plane.  Here every (Gaussian, ray) pair is the closed-form integral
over the whole line; in cone beam a pair whose closest approach lies at or behind the source contributes 0, a pair is only
skipped when its exponent q exceeds 32 (below exp(-16) of the Gaussian's peak), and nothing is culled at a near plane.  The
rays are the [V,12] parameters of the volume projectors (projector.py), in world coordinates, so a detector the rasterizer's
camera cannot describe (shifted, tilted) can be projected with ``project_gaussians_rays``.

``integrate_rays`` is the same line integral along rays that are no detector's: any [..., 3] starts and directions, on the
kernels of csrc/gaussian_bundle.hip and csrc/gaussian_bundle_bwd.hip (``r2_integrate_gaussians`` and its backward), or, with
``method="leaves"``, of csrc/gaussian_leaves.hip and csrc/gaussian_leaves_bwd.hip (``r2_integrate_gaussians_leaves``).

``project_gaussians_jvp`` / ``project_gaussians_rays_jvp`` apply the projector's Jacobian forwards, to a tangent of the cloud,
of the rays, or both, on the kernels of csrc/gaussian_tangent.hip (``r2_project_gaussians_jvp``,
``r2_project_gaussians_ray_jacobian``); gauss_newton.py and ``geometry.refine_geometry_lm`` build their solvers on them.

``plan_projection`` / ``plan_projection_rays`` build a ``ProjectionPlan``, the per-tile Gaussian lists of one (rays, cloud), on
the kernels of csrc/gaussian_plan.hip; the pixel-major operators take it as ``plan=`` and write the same bits sooner.
"""
import torch

from . import _lib
from . import projector
from ._boundary import _F32, call, cloud, f32c, require_gpu, workspace


def world_ray_params(views):
    """[V,12] float32 ray parameters {a, p00, pu, pv} of ``views`` (``scene.View`` list) in world coordinates: what
    ``projector.ray_params`` gives for a unit voxel grid whose index coordinates are the world's."""
    return projector.ray_params(views, (1.0, 1.0, 1.0), (0.0, 0.0, 0.0), (1, 1, 1))


_PLAN_SOURCES = ("rays", "xyz", "density", "scaling", "rotation")


class ProjectionPlan:
    """The per-tile Gaussian lists of one (rays, detector, cloud): what ``plan_projection_rays`` returns and the ``plan=``
    keyword of the pixel-major operators takes (include/r2hip.h, "projection plans", has the layout).

    ``offsets`` int64 [V T + 1] and ``ids`` int32 [instances], both on the GPU (``lists()`` returns the two); ``instances``,
    ``V``, ``H``, ``W``, ``cone``, ``P``, ``scale_modifier`` as it was built.  The plan keeps references to the rays tensor
    and the four cloud tensors it was built from and records their shapes and ``_version`` counters: a consumer that is handed
    other tensors, tensors that were written in place since, or another detector, beam or scale modifier raises ValueError
    (``check``) instead of projecting with stale lists."""

    def __init__(self, offsets, ids, instances, V, H, W, cone, P, scale_modifier, sources):
        self.offsets, self.ids, self.instances = offsets, ids, int(instances)
        self.V, self.H, self.W, self.cone, self.P, self.scale_modifier = V, H, W, bool(cone), P, float(scale_modifier)
        self._sources = tuple((t, tuple(t.shape), t._version) for t in sources)
        self._view_params = None   # plan_projection: the [V,12] host parameters of the views it was built from

    def lists(self):
        """-> (offsets, ids)."""
        return self.offsets, self.ids

    def check(self, rays, cone, H, W, xyz, density, scaling, rotation, scale_modifier):
        """ValueError, naming what changed, unless the arguments are the ones the plan was built from."""
        changed = [n for n, a, b in (("H", int(H), self.H), ("W", int(W), self.W), ("cone", bool(cone), self.cone),
                                     ("scale_modifier", float(scale_modifier), self.scale_modifier)) if a != b]
        for name, t, (src, shape, version) in zip(_PLAN_SOURCES, (rays, xyz, density, scaling, rotation), self._sources):
            if t is not src:
                changed.append("%s (another tensor)" % name)
            elif tuple(t.shape) != shape:
                changed.append("%s (shape %s, planned with %s)" % (name, tuple(t.shape), shape))
            elif t._version != version:
                changed.append("%s (written in place since)" % name)
        if changed:
            raise ValueError("the projection plan is stale or belongs to other arguments: %s changed; build a new plan"
                             % ", ".join(changed))

    def _args(self):
        return self.offsets.data_ptr(), self.ids.data_ptr(), self.ids.numel()


def _call_planned(name, plan, dev, *args):
    """``_boundary.call`` of the entry ``name``, or, with a plan, of ``name + "_planned"``: the planned entries take the plan's
    three arguments last before the stream (``_lib._SIGNATURES``)."""
    if plan is None:
        return call(name, dev, *args)
    return call(name + "_planned", dev, *args, *plan._args())


def _plan_count(rays, cone, H, W, x, d, s, r, scale_modifier):
    """``r2_project_gaussians_plan_count`` on kernel-ready tensors -> (offsets, the workspace that holds the table)."""
    V, P, dev = rays.shape[0], x.shape[0], x.device
    T = ((H + 15) // 16) * ((W + 15) // 16)
    offsets = torch.empty((V * T + 1,), dtype=torch.int64, device=dev)
    ws = workspace(_lib.lib().r2_project_gaussians_plan_workspace_bytes(V, H, W, P), dev, at_least=1)
    call("r2_project_gaussians_plan_count", dev, V, H, W, rays, cone, P, x, d, s, float(scale_modifier), r, offsets, ws, ws.numel())
    return offsets, ws


def _plan_fill(rays, cone, H, W, x, d, s, r, scale_modifier, offsets, ws, instances):
    """``r2_project_gaussians_plan_fill`` after ``_plan_count`` -> ids [instances]."""
    V, P, dev = rays.shape[0], x.shape[0], x.device
    ids = torch.empty((instances,), dtype=torch.int32, device=dev)
    call("r2_project_gaussians_plan_fill", dev, V, H, W, rays, cone, P, x, d, s, float(scale_modifier), r, offsets,
         ids if instances else None, instances, ws, ws.numel())
    return ids


@torch.no_grad()
def plan_projection_rays(rays, cone, H, W, xyz, density, scaling, rotation, scale_modifier=1.0):
    """The ``ProjectionPlan`` of ``project_gaussians_rays`` on the same arguments: for every 16 x 16 tile of every view the
    ascending list of the Gaussians whose detector rectangle meets it.  Hand it to the pixel-major operators (``plan=``):
    ``project_gaussians_rays`` (the forward and its ray backward), ``project_gaussians_rays_jvp``, ``geometry.ray_jacobian``,
    ``uncertainty.projection_variance_rays``; they then walk a tile's list where they otherwise test all P Gaussians per tile,
    and write the same bits.  Worth it when the same cloud is projected on the same rays more than once
    (``gauss_newton.gauss_newton_step(planned=True)``); DESIGN.md section 4, "Projection plans", has the break-even.

    Building costs two groups of launches and ONE host read between them, of the instance count that sizes ``ids``: unlike
    the operators themselves, this function synchronises with the device.  ``rays`` should be a tensor (the plan records its
    identity; an array is converted anew on every call and can never match).  Deterministic: building twice gives equal
    tensors, and a view's lists do not depend on the other views."""
    rays, H, W = check_projection_arguments(rays, H, W, xyz, density, scaling, rotation)
    V, P, dev = rays.shape[0], xyz.shape[0], xyz.device
    rdev = projector.device_rays(rays.detach(), dev)
    x, d, s, r = cloud(xyz, density, scaling, rotation)
    c = int(bool(cone))
    offsets, ws = _plan_count(rdev, c, H, W, x, d, s, r, scale_modifier)
    instances = int(offsets[-1])   # the one host read
    ids = _plan_fill(rdev, c, H, W, x, d, s, r, scale_modifier, offsets, ws, instances)
    return ProjectionPlan(offsets, ids, instances, V, H, W, cone, P, scale_modifier, (rays, xyz, density, scaling, rotation))


def plan_projection(views, xyz, density, scaling, rotation, scale_modifier=1.0):
    """``plan_projection_rays`` on ``views`` (``scene.View`` list: one detector size, one beam mode), for the operators that
    take views.  Those check that the views they are given have the ray parameters the plan was built from."""
    views, H, W = projector.check_views(views)
    params = world_ray_params(views)
    plan = plan_projection_rays(torch.from_numpy(params), views[0].mode == 1, H, W, xyz, density, scaling, rotation, scale_modifier)
    plan._view_params = params.copy()
    return plan


def _view_rays(views, plan):
    """The rays tensor of ``views``: a new one without a plan, else the plan's own, after the views were compared with it."""
    params = world_ray_params(views)
    if plan is None:
        return torch.from_numpy(params)
    if not isinstance(plan, ProjectionPlan):
        raise ValueError("plan must be a ProjectionPlan, got %r" % type(plan).__name__)
    if plan._view_params is None:
        raise ValueError("the projection plan was built from rays (plan_projection_rays): use the operator that takes rays")
    if plan._view_params.shape != params.shape or not (plan._view_params == params).all():
        raise ValueError("the projection plan is stale or belongs to other arguments: views changed; build a new plan")
    return plan._sources[0][0]


def _checked_plan(plan, rays, cone, H, W, xyz, density, scaling, rotation, scale_modifier):
    """None, or ``plan`` after its staleness check against the caller's own tensors."""
    if plan is None:
        return None
    if not isinstance(plan, ProjectionPlan):
        raise ValueError("plan must be a ProjectionPlan, got %r" % type(plan).__name__)
    plan.check(rays, cone, H, W, xyz, density, scaling, rotation, scale_modifier)
    return plan


class _ProjectGaussians(torch.autograd.Function):
    @staticmethod
    def forward(ctx, xyz, density, scaling, rotation, rays, cone, H, W, scale_modifier, out, plan=None):
        V, P = rays.shape[0], xyz.shape[0]
        x, d, s, r = cloud(xyz, density, scaling, rotation)
        rays = rays.detach()
        _call_planned("r2_project_gaussians", plan, x.device, V, H, W, rays, cone, P, x, d, s, float(scale_modifier), r, out)
        ctx.save_for_backward(x, d, s, r, rays)
        ctx.args = (cone, H, W, float(scale_modifier))
        ctx.plan = plan
        ctx.mark_dirty(out)
        return out

    @staticmethod
    def backward(ctx, G):
        x, d, s, r, rays = ctx.saved_tensors
        cone, H, W, mod = ctx.args
        V, P = rays.shape[0], x.shape[0]
        G = f32c(G)
        gx = gd = gs = gr = grays = None
        if any(ctx.needs_input_grad[:4]):
            gx, gd, gs, gr = torch.empty_like(x), torch.empty_like(d), torch.empty_like(s), torch.empty_like(r)
            call("r2_project_gaussians_backward", x.device, V, H, W, rays, cone, P, x, d, s, mod, r, G, gx, gd, gs, gr)
        if ctx.needs_input_grad[4]:
            grays = torch.empty_like(rays)
            ws = workspace(_lib.lib().r2_project_gaussians_rays_backward_workspace_bytes(V, H, W), x.device, at_least=1)
            _call_planned("r2_project_gaussians_rays_backward", ctx.plan, x.device, V, H, W, rays, cone, P, x, d, s, mod, r, G, grays,
                          ws, ws.numel())
        return gx, gd, gs, gr, grays, None, None, None, None, None, None


def check_projection_arguments(rays, H, W, xyz, density, scaling, rotation):
    """The argument checks every operator on (rays, detector, cloud) shares: ``rays`` [V,12] with V >= 1, a detector of at least
    one pixel, the four parameter tensors of one P on one GPU.  -> (rays as a tensor, H, W), or ValueError."""
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
    return rays, H, W


def project_gaussians_rays(rays, cone, H, W, xyz, density, scaling, rotation, scale_modifier=1.0, out=None, plan=None):
    """Exact projections [V,H,W] (GPU, float32) of the cloud ``xyz`` [P,3], ``density`` [P,1] or [P], ``scaling`` [P,3],
    ``rotation`` [P,4] (activated values; the quaternion is used as it comes) along caller-supplied rays: ``rays`` [V,12]
    {a, p00, pu, pv} in world coordinates (include/r2hip.h), ``cone`` the beam (True: from the source a through the pixel
    points; False: through the pixel points along a).  Differentiable in the four parameter tensors, and in ``rays`` when they
    require grad (``r2_project_gaussians_rays_backward``, launched only then): a ``rays`` tensor on the device or on the host,
    of any float dtype, receives its gradient where and as it is.  No host synchronisation (host rays that require grad are
    copied synchronously); ``out`` may be a preallocated contiguous float32 GPU tensor [V,H,W].
    ``plan``: a ``ProjectionPlan`` built from these very tensors (``plan_projection_rays``); the forward and the ray backward
    then walk the plan's lists (``r2_project_gaussians_planned``, ``r2_project_gaussians_rays_backward_planned``), the
    parameter backward is unchanged, and every result is the same bits.  A stale plan raises ValueError."""
    rays, H, W = check_projection_arguments(rays, H, W, xyz, density, scaling, rotation)
    plan = _checked_plan(plan, rays, cone, H, W, xyz, density, scaling, rotation, scale_modifier)
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
    return _ProjectGaussians.apply(xyz, density, scaling, rotation, rays, int(bool(cone)), H, W, float(scale_modifier), out, plan)


def project_gaussians(views, xyz, density, scaling, rotation, scale_modifier=1.0, out=None, plan=None):
    """Exact projections [V,H,W] of the cloud on ``views`` (``scene.View`` list: one detector size, one beam mode), registered
    to the rasterizer's image of the same view.  See ``project_gaussians_rays``; ``plan``: from ``plan_projection``."""
    views, H, W = projector.check_views(views)
    return project_gaussians_rays(_view_rays(views, plan), views[0].mode == 1, H, W, xyz, density, scaling, rotation,
                                  scale_modifier, out, plan)


def _ray_jacobian(rays, cone, H, W, xyz, density, scaling, rotation, scale_modifier=1.0, plan=None):
    """``geometry.ray_jacobian``, where its documentation is: [V,6,H,W] on ``r2_project_gaussians_ray_jacobian``, or, with a
    plan, on ``r2_project_gaussians_ray_jacobian_planned``."""
    rays, H, W = check_projection_arguments(rays, H, W, xyz, density, scaling, rotation)
    plan = _checked_plan(plan, rays, cone, H, W, xyz, density, scaling, rotation, scale_modifier)
    V, P, dev = rays.shape[0], xyz.shape[0], xyz.device
    rays = projector.device_rays(rays.detach(), dev)
    x, d, s, r = cloud(xyz, density, scaling, rotation)
    out = torch.empty((V, 6, H, W), dtype=_F32, device=dev)
    _call_planned("r2_project_gaussians_ray_jacobian", plan, dev, V, H, W, rays, int(bool(cone)), P, x, d, s, float(scale_modifier),
                  r, out)
    return out


def contract_ray_jacobian(jac, ray_tangent, cone):
    """The ray Jacobian ``jac`` [V,6,H,W] (``geometry.ray_jacobian``) applied to a tangent ``ray_tangent`` [V,12] of the rays
    {a, p00, pu, pv} -> [V,H,W] float64: the pixel point is P = p00 + c pu + r pv, so t_P = t_p00 + c t_pu + r t_pv; cone beam
    has ds = t_a, dd = t_P - t_a, parallel beam ds = t_P, dd = t_a.  Plain torch in float64 on the device of ``jac``."""
    V, _, H, W = jac.shape
    t = ray_tangent.to(device=jac.device, dtype=torch.float64)
    c = torch.arange(W, dtype=torch.float64, device=jac.device)[None, None, :, None]
    r = torch.arange(H, dtype=torch.float64, device=jac.device)[None, :, None, None]
    tP = t[:, None, None, 3:6] + c * t[:, None, None, 6:9] + r * t[:, None, None, 9:12]
    ta = t[:, None, None, 0:3].expand_as(tP)
    ds, dd = (ta, tP - ta) if cone else (tP, ta)
    j = jac.to(torch.float64)
    return (j[:, 0:3].permute(0, 2, 3, 1) * ds).sum(-1) + (j[:, 3:6].permute(0, 2, 3, 1) * dd).sum(-1)


@torch.no_grad()
def project_gaussians_rays_jvp(rays, cone, H, W, xyz, density, scaling, rotation, tangents=None, ray_tangent=None,
                               scale_modifier=1.0, plan=None):
    """The directional derivative [V,H,W] (GPU, float32) of ``project_gaussians_rays`` on the same arguments: J t for a tangent
    of the cloud, of the rays, or of both (their sum).  ``tangents``: a 4-tuple shaped like the cloud (xyz [P,3], density
    [P,1] or [P], scaling [P,3], rotation [P,4]), in the parameters of the projector's gradient (the scales as given, the
    quaternion as it comes): one launch of ``r2_project_gaussians_jvp``, the cost of ``uncertainty.projection_variance``.
    ``ray_tangent`` [V,12]: one launch of ``r2_project_gaussians_ray_jacobian`` (``geometry.ray_jacobian``), contracted in
    torch with every pixel's (ds, dd) (``contract_ray_jacobian``).  At least one of the two must be given.  Which pairs are
    summed is piecewise constant and not differentiated, as in the backward, whose transpose this is:
    <G, J t> = <J^T G, t> up to rounding.  The result is not attached to autograd.  No host synchronisation.
    ``plan``: a ``ProjectionPlan`` built from these very tensors; both launches then walk its lists
    (``r2_project_gaussians_jvp_planned``, ``r2_project_gaussians_ray_jacobian_planned``) and give the same bits."""
    if tangents is None and ray_tangent is None:
        raise ValueError("give tangents, ray_tangent or both")
    rays, H, W = check_projection_arguments(rays, H, W, xyz, density, scaling, rotation)
    plan = _checked_plan(plan, rays, cone, H, W, xyz, density, scaling, rotation, scale_modifier)
    V, P, dev = rays.shape[0], xyz.shape[0], xyz.device
    out = None
    if tangents is not None:
        from .uncertainty import _check_group_tuple
        tx, td, ts, tr = _check_group_tuple(tangents, P, dev, "tangents")
        rdev = projector.device_rays(rays.detach(), dev)
        x, d, s, r = cloud(xyz, density, scaling, rotation)
        out = torch.empty((V, H, W), dtype=_F32, device=dev)
        _call_planned("r2_project_gaussians_jvp", plan, dev, V, H, W, rdev, int(bool(cone)), P, x, d, s, float(scale_modifier), r,
                      tx, td, ts, tr, out)
    if ray_tangent is not None:
        ray_tangent = torch.as_tensor(ray_tangent)
        if tuple(ray_tangent.shape) != (V, 12):
            raise ValueError("ray_tangent must be [%d,12], got %s" % (V, tuple(ray_tangent.shape)))
        jac = _ray_jacobian(rays, cone, H, W, xyz, density, scaling, rotation, scale_modifier, plan)
        part = contract_ray_jacobian(jac, ray_tangent.detach(), bool(cone)).to(_F32)
        out = part if out is None else out + part
    return out


def project_gaussians_jvp(views, xyz, density, scaling, rotation, tangents=None, ray_tangent=None, scale_modifier=1.0, plan=None):
    """``project_gaussians_rays_jvp`` on ``views`` (``scene.View`` list: one detector size, one beam mode); ``plan``: from
    ``plan_projection``."""
    views, H, W = projector.check_views(views)
    return project_gaussians_rays_jvp(_view_rays(views, plan), views[0].mode == 1, H, W, xyz, density, scaling, rotation, tangents,
                                      ray_tangent, scale_modifier, plan)


_BLOCKS = ("r2_integrate_gaussians", "r2_integrate_gaussians_backward", "r2_integrate_gaussians_workspace_bytes")
_LEAVES = ("r2_integrate_gaussians_leaves", "r2_integrate_gaussians_leaves_backward",
           "r2_integrate_gaussians_leaves_workspace_bytes")


def _integrate_forward(ctx, entries, origins, directions, xyz, density, scaling, rotation, scale_modifier, half_line, perm,
                       gperm=None):
    """origins, directions [N,3] -> [N] through the C entries ``entries``.  ``perm`` (or None): the order the kernels see the
    rays in; ``gperm`` (or None): the order they see the Gaussians in.  Values and gradients come back in the caller's
    orders, by gathers alone."""
    from .field import inverse_permutation
    N, P = origins.shape[0], xyz.shape[0]
    x, d, s, r = cloud(xyz, density, scaling, rotation)
    ginv = None
    if gperm is not None:
        x, d, s, r = (t[gperm].contiguous() for t in (x, d, s, r))
        ginv = inverse_permutation(gperm)
    rays = torch.cat([origins.detach().to(_F32), directions.detach().to(_F32)], 1)
    inv = None
    if perm is not None:
        rays, inv = rays[perm].contiguous(), inverse_permutation(perm)
    out = torch.empty((N,), dtype=_F32, device=x.device)
    ws = workspace(getattr(_lib.lib(), entries[2])(N, P), x.device, at_least=1)
    call(entries[0], x.device, N, rays, half_line, P, x, d, s, float(scale_modifier), r, out, ws, ws.numel())
    ctx.save_for_backward(rays, x, d, s, r, perm, inv, ginv)
    ctx.args = (float(scale_modifier), half_line)
    return out if inv is None else out[inv]


def _integrate_backward(ctx, entries, G):
    rays, x, d, s, r, perm, inv, ginv = ctx.saved_tensors
    mod, half_line = ctx.args
    N, P = rays.shape[0], x.shape[0]
    G = f32c(G)
    if perm is not None:
        G = G[perm].contiguous()
    gx, gd, gs, gr = torch.empty_like(x), torch.empty_like(d), torch.empty_like(s), torch.empty_like(r)
    grays = torch.empty_like(rays) if ctx.needs_input_grad[0] or ctx.needs_input_grad[1] else None
    ws = workspace(getattr(_lib.lib(), entries[2])(N, P), x.device, at_least=1)
    call(entries[1], x.device, N, rays, half_line, P, x, d, s, mod, r, G, gx, gd, gs, gr, grays, ws, ws.numel())
    if ginv is not None:
        gx, gd, gs, gr = gx[ginv], gd[ginv], gs[ginv], gr[ginv]
    go = gdir = None
    if grays is not None:
        if inv is not None:
            grays = grays[inv]
        go, gdir = grays[:, :3], grays[:, 3:]
    return go, gdir, gx, gd, gs, gr


class _IntegrateRays(torch.autograd.Function):
    """origins, directions [N,3] -> [N] on r2_integrate_gaussians (culling by blocks of rays)."""

    @staticmethod
    def forward(ctx, origins, directions, xyz, density, scaling, rotation, scale_modifier, half_line, perm):
        return _integrate_forward(ctx, _BLOCKS, origins, directions, xyz, density, scaling, rotation, scale_modifier, half_line, perm)

    @staticmethod
    def backward(ctx, G):
        return _integrate_backward(ctx, _BLOCKS, G) + (None, None, None)


class _IntegrateRaysLeaves(torch.autograd.Function):
    """origins, directions [N,3] -> [N] on r2_integrate_gaussians_leaves (culling by leaves of Gaussians); ``gperm`` (or
    None): the order of the Gaussians the kernels see."""

    @staticmethod
    def forward(ctx, origins, directions, xyz, density, scaling, rotation, scale_modifier, half_line, perm, gperm):
        return _integrate_forward(ctx, _LEAVES, origins, directions, xyz, density, scaling, rotation, scale_modifier, half_line, perm,
                                  gperm)

    @staticmethod
    def backward(ctx, G):
        return _integrate_backward(ctx, _LEAVES, G) + (None, None, None, None)


def cloud_order(xyz, scaling, scale_modifier=1.0):
    """Permutation [P] (int64) that makes leaves of 64 consecutive Gaussians compact: a stable sort by (size class, 30-bit
    Morton key of the mean), large Gaussians first.  The size class is floor(log2(diagonal of the box of the means /
    radius)) with the radius proxy ``scale_modifier`` * max scale * 5.72 (the bounding sphere of a unit quaternion): Gaussians
    within a factor two in size share a class, so that one large Gaussian does not inflate the box of a leaf of small ones.
    The Morton key has 10 bits for each coordinate of the mean in the box of the means.  Rows with a non-finite mean or
    scale, or no positive radius, get key 0 and come first.  It affects the cost of ``integrate_rays(method="leaves")``
    alone.  torch ops only, on the tensors' device (CPU tensors too); no host synchronisation."""
    m, s = xyz.detach().to(torch.float64), scaling.detach().to(torch.float64)
    P = m.shape[0]
    if P == 0:
        return torch.arange(0, device=m.device)
    radius = float(scale_modifier) * s.amax(1) * 5.72
    good = torch.isfinite(m).all(1) & torch.isfinite(s).all(1) & torch.isfinite(radius) & (radius > 0)
    big = torch.finfo(torch.float64).max
    lo = torch.where(good[:, None], m, torch.full_like(m, big)).amin(0)
    hi = torch.where(good[:, None], m, torch.full_like(m, -big)).amax(0)
    ext = torch.where(hi > lo, hi - lo, torch.ones_like(lo))   # no good row, or a flat box: any positive number
    diag = torch.where(hi > lo, hi - lo, torch.zeros_like(lo)).norm()
    safe = torch.where(good, radius, torch.ones_like(radius))
    cls = torch.log2(diag / safe).floor().clamp(0.0, 60.0)     # log2(0) = -inf clamps to 0
    cell = ((torch.where(good[:, None], m, lo.expand_as(m)) - lo) / ext * 1024.0).floor().clamp(0.0, 1023.0).to(torch.int64)
    key = (cls.to(torch.int64) + 1) << 30
    for bit in range(10):
        for j in range(3):
            key = key | (((cell[:, j] >> bit) & 1) << (3 * bit + j))
    key = torch.where(good, key, torch.zeros_like(key))
    return torch.sort(key, stable=True)[1]


def ray_order(origins, directions, xyz):
    """Permutation [N] (int64) that makes blocks of consecutive rays coherent: a stable sort by a 30-bit Morton key of the
    two points where a ray's line enters and leaves a sphere around the cloud (5 bits for each of the six coordinates; a line
    that misses the sphere takes its closest point twice), so that rays next to each other in the order are close all the way
    through the cloud.  The sphere: the centre of the box of the finite means, 0.55 of its diagonal.  Rays with a
    non-finite component or no direction get key 0.  torch ops only, on the rays' device; no host synchronisation."""
    o, d, m = origins.detach().to(torch.float64), directions.detach().to(torch.float64), xyz.detach().to(torch.float64)
    if o.shape[0] == 0 or m.shape[0] == 0:
        return torch.arange(o.shape[0], device=o.device)
    big = torch.finfo(torch.float64).max
    fin = torch.isfinite(m).all(1, keepdim=True)
    lo = torch.where(fin, m, torch.full_like(m, big)).amin(0)
    hi = torch.where(fin, m, torch.full_like(m, -big)).amax(0)
    some = (hi >= lo).all()
    centre = torch.where(some, 0.5 * lo + 0.5 * hi, torch.zeros_like(lo))
    radius = torch.where(some, 0.55 * (hi - lo).norm(), torch.ones_like(lo[0])) + 1e-30
    length = d.norm(dim=1, keepdim=True)
    good = torch.isfinite(o).all(1, keepdim=True) & torch.isfinite(d).all(1, keepdim=True) & (length > 0) & torch.isfinite(length)
    h = torch.where(good, d / torch.where(good, length, torch.ones_like(length)), torch.zeros_like(d))
    e = torch.where(good, o - centre, torch.zeros_like(o))
    t = -(e * h).sum(1, keepdim=True)
    near = e + t * h
    half = (radius * radius - (near * near).sum(1, keepdim=True)).clamp_min(0.0).sqrt()
    ends = torch.cat([near - half * h, near + half * h], 1)
    cell = ((ends / radius + 1.0) * 16.0).floor().clamp_(0, 31)
    cell = torch.where(good, cell, torch.zeros_like(cell)).to(torch.int64)
    key = torch.zeros_like(cell[:, 0])
    for bit in range(5):
        for j in range(6):
            key = key | (((cell[:, j] >> bit) & 1) << (6 * bit + j))
    return torch.sort(key, stable=True)[1]


def integrate_rays(origins, directions, xyz, density, scaling, rotation, scale_modifier=1.0, half_line=False, sort=False,
                   method="blocks", order=False):
    """Exact line integrals [...] (GPU, float32) of the cloud ``xyz`` [P,3], ``density`` [P,1] or [P], ``scaling`` [P,3],
    ``rotation`` [P,4] (activated values; the quaternion is used as it comes) along the rays ``origins`` + t ``directions``,
    both [..., 3] of one shape, in world coordinates; the directions need not be normalised.  A pair is the projector's:
    the integral over the whole line, and with ``half_line`` the cone rule (a Gaussian whose closest approach lies at or
    behind the origin contributes 0), so ``integrate_rays(*geometry.pixel_rays(rays, cone, H, W), ..., half_line=cone)`` is
    the image of ``project_gaussians_rays`` up to which pairs beyond q = 32 are summed.  Differentiable in the four parameter
    tensors, and in ``origins`` and ``directions`` when they require grad.  No host synchronisation.

    The kernels cull by blocks of 256 consecutive rays (include/r2hip.h: r2_integrate_gaussians), so coherent inputs -- the
    pixels of a detector tile, the columns of a curved detector -- cull well as they are.  ``sort=True`` is meant for
    scattered rays: it orders them by ``ray_order`` before the kernels see them and un-permutes values and gradients.
    Which pairs a ray sums does not depend on the other rays, so sorting changes the cost alone: the values and the ray
    gradients are the same bits.

    ``method``: "blocks" (the default) is the path above; "leaves" culls from the other side, by leaves of 64 consecutive
    Gaussians (include/r2hip.h: r2_integrate_gaussians_leaves): one wave per ray walks only the leaves its line meets, so the
    cost follows the number of rays and no ray waits for another ray's Gaussians.  "blocks" suits whole detectors, tiles and
    other coherent rays, where 256 rays share every Gaussian they stage; "leaves" suits scattered rays, such as a random
    subset of the pixels of many views.  The rule that decides which pairs are summed is the same; the sums associate
    differently, so the two methods agree to rounding.  "leaves" culls well when the index order of the cloud is spatially
    coherent and keeps large Gaussians together, and any other order costs time and nothing else: ``order=True`` (valid with
    "leaves" only) gathers the four parameter tensors by ``cloud_order`` before the kernels and scatters the four gradients
    back.  Summation order follows the Gaussian order, so values with and without ``order`` differ by rounding, not by which
    pairs are summed.  A cloud that is integrated many times is better ordered once, outside.  ``sort`` keeps its meaning with
    "leaves" and, each ray being a wave of its own there, buys little."""
    if method not in ("blocks", "leaves"):
        raise ValueError("method must be 'blocks' or 'leaves', got %r" % (method,))
    if order and method != "leaves":
        raise ValueError("order=True is valid with method='leaves' only")
    for name, t in (("origins", origins), ("directions", directions)):
        if not isinstance(t, torch.Tensor) or t.dim() < 1 or t.shape[-1] != 3:
            raise ValueError("%s must be a tensor [..., 3], got %s" % (name, tuple(getattr(t, "shape", ()))))
    if origins.shape != directions.shape:
        raise ValueError("origins and directions differ in shape: %s, %s" % (tuple(origins.shape), tuple(directions.shape)))
    require_gpu(origins, "origins")
    require_gpu(directions, "directions")
    from .field import _check_cloud
    _check_cloud(xyz, density, scaling, rotation)
    if origins.device != xyz.device or directions.device != xyz.device:
        raise ValueError("the rays are on %s and %s, xyz on %s" % (origins.device, directions.device, xyz.device))
    o, d = origins.reshape(-1, 3), directions.reshape(-1, 3)
    if o.shape[0] >= (1 << 31):
        raise ValueError("fewer than 2^31 rays, got %d" % o.shape[0])
    perm = ray_order(o, d, xyz) if sort else None
    if method == "leaves":
        gperm = cloud_order(xyz, scaling, scale_modifier) if order else None
        out = _IntegrateRaysLeaves.apply(o, d, xyz, density, scaling, rotation, float(scale_modifier), int(bool(half_line)), perm,
                                         gperm)
    else:
        out = _IntegrateRays.apply(o, d, xyz, density, scaling, rotation, float(scale_modifier), int(bool(half_line)), perm)
    return out.reshape(origins.shape[:-1])
