"""Scan geometry as differentiable ray parameters, and its refinement against the model's exact projection.

``scan_rays`` builds the [V,12] world rays {a, p00, pu, pv} (include/r2hip.h) of a circular scan whose detector may be shifted
in its plane, rolled about its normal and tilted about its two axes, view by view, with jittered angles -- what
``scene.make_view`` (and with it ``gaussian_projector.world_ray_params``) cannot describe.  It is torch, float64 inside, and
differentiable in every continuous argument; ``gaussian_projector.project_gaussians_rays`` is differentiable in its rays
(``r2_project_gaussians_rays_backward``), so a loss on exact projections reaches the geometry.  ``refine_geometry`` is that
loop: the cloud held fixed, Adam on the chosen geometry parameters.  ``refine_geometry_lm`` solves the same least-squares
problem by Levenberg-Marquardt, on ``ray_jacobian``: every pixel's derivative in its own ray
(``r2_project_gaussians_ray_jacobian``), through which any number of geometry parameters chains in torch.

``pixel_rays`` turns [V,12] views into per-pixel starts and directions, the whole detector or chosen pixels, and
``curved_detector_rays`` builds those of an equiangular cylindrical detector, for ``gaussian_projector.integrate_rays``,
which takes any rays and is differentiable in them.
"""
import torch

_F64 = torch.float64


def _per_view(x, V, device):
    """A scalar or a per-view tensor [V] as a float64 tensor [V] on ``device``."""
    t = x.to(device=device, dtype=_F64) if isinstance(x, torch.Tensor) else torch.as_tensor(x, dtype=_F64, device=device)
    if t.dim() > 1 or (t.dim() == 1 and t.shape[0] not in (1, V)):
        raise ValueError("a geometry argument must be a scalar or a tensor [V] with V = %d, got shape %s" % (V, tuple(t.shape)))
    return t.reshape(-1).expand(V)


def _several(x, n, name, V, device):
    if isinstance(x, torch.Tensor) and x.dim() >= 1 and x.shape[-1] == n:
        x = x.unbind(-1)
    if len(x) != n:
        raise ValueError("%s must have %d entries" % (name, n))
    return [_per_view(e, V, device) for e in x]


def scan_rays(angles, DSO, DSD, dDetector, nDetector, offDetector=(0.0, 0.0), roll=0.0, tilt=(0.0, 0.0),
              offOrigin=(0.0, 0.0, 0.0), mode="cone", d_angle=None):
    """[V,12] float64 world rays {a, p00, pu, pv} of a circular scan about the z axis.

    ``angles`` [V] (plus ``d_angle``, a per-view correction, when given); ``DSO`` / ``DSD`` the source-to-axis and
    source-to-detector distances; ``dDetector`` = (row pitch, column pitch) and ``nDetector`` = (H, W), in the order of the
    scanner configs (``scene.CONE_BEAM``: sDetector = nDetector * dDetector); lengths in world (scene) units, so a raw scanner
    config is scaled first (``scanner_args``).  Every continuous argument is a scalar or a per-view tensor [V] (the pairs and
    the triple: sequences of such, or tensors [..., n]) and is differentiated when it requires grad.

    The source of view i sits at DSO (cos t, sin t, 0), t = angles_i + d_angle_i; the detector frame is
    eu = (-sin t, cos t, 0) (columns), ev = (0, 0, -1) (rows), en = (-cos t, -sin t, 0) (from the source to the axis), as
    ``scene.make_view`` has it.  The detector is rotated about its centre by Rn(roll) Ru(tilt[0]) Rv(tilt[1]) (about its
    normal, then its column axis, then its row axis, angles in radians, right-handed in (eu, ev, en)), then moved by
    offDetector = (along its rows' direction ev', along its columns' direction eu') in its own rotated plane.  ``offOrigin``
    (x, y, z) is the position of the object relative to the rotation centre: in world coordinates, which are the object's,
    source and detector move by -offOrigin.  Pixel (r, c) is the point p00 + c pu + r pv.

    ``mode="cone"``: a = the source, and the detector is drawn towards the source by the factor 1 / DSD (the rays are the same
    lines), which is where ``world_ray_params`` puts it.  ``mode="parallel"``: a = en, the common direction, and the detector
    plane passes through the source position; DSD does not enter.  At offDetector = roll = tilt = offOrigin = 0 the result
    restates ``world_ray_params([make_view(t, nDetector, scanner)])`` for the lengths ``scanner_args`` takes from ``scanner``.
    """
    if mode not in ("cone", "parallel"):
        raise ValueError("mode must be 'cone' or 'parallel', got %r" % (mode,))
    H, W = int(nDetector[0]), int(nDetector[1])
    if H < 1 or W < 1:
        raise ValueError("the detector must have at least one pixel, got %d x %d" % (H, W))
    tensors = [x for x in (angles, d_angle, DSO, DSD, roll) if isinstance(x, torch.Tensor)]
    for group in (dDetector, offDetector, tilt, offOrigin):
        tensors += [x for x in ([group] if isinstance(group, torch.Tensor) else group) if isinstance(x, torch.Tensor)]
    device = tensors[0].device if tensors else torch.device("cpu")
    ang = (angles.to(device=device, dtype=_F64) if isinstance(angles, torch.Tensor)
           else torch.as_tensor(angles, dtype=_F64, device=device)).reshape(-1)
    V = ang.shape[0]
    if V < 1:
        raise ValueError("no views")
    if d_angle is not None:
        ang = ang + _per_view(d_angle, V, device)
    DSO, DSD, roll = (_per_view(x, V, device) for x in (DSO, DSD, roll))
    dV, dU = _several(dDetector, 2, "dDetector", V, device)
    oV, oU = _several(offDetector, 2, "offDetector", V, device)
    tU, tV = _several(tilt, 2, "tilt", V, device)
    org = torch.stack(_several(offOrigin, 3, "offOrigin", V, device), 1)
    c, s = torch.cos(ang), torch.sin(ang)
    zero, one = torch.zeros_like(c), torch.ones_like(c)
    eu = torch.stack([-s, c, zero], 1)
    ev = torch.stack([zero, zero, -one], 1)
    en = torch.stack([-c, -s, zero], 1)
    # the first two columns of Rn(roll) Ru(tU) Rv(tV) in the frame (eu, ev, en)
    cr, sr, cu, su, cv, sv = torch.cos(roll), torch.sin(roll), torch.cos(tU), torch.sin(tU), torch.cos(tV), torch.sin(tV)
    col_u = (cr * cv - sr * su * sv, sr * cv + cr * su * sv, -cu * sv)
    col_v = (-sr * cu, cr * cu, su)
    fu = col_u[0][:, None] * eu + col_u[1][:, None] * ev + col_u[2][:, None] * en
    fv = col_v[0][:, None] * eu + col_v[1][:, None] * ev + col_v[2][:, None] * en
    src = DSO[:, None] * torch.stack([c, s, zero], 1) - org
    centre = src + DSD[:, None] * en if mode == "cone" else src
    centre = centre + oU[:, None] * fu + oV[:, None] * fv
    pu, pv = dU[:, None] * fu, dV[:, None] * fv
    p00 = centre + (0.5 - 0.5 * W) * pu + (0.5 - 0.5 * H) * pv
    if mode == "cone":
        k = 1.0 / DSD[:, None]
        return torch.cat([src, src + (p00 - src) * k, pu * k, pv * k], 1)
    return torch.cat([en, p00, pu, pv], 1)


def pixel_rays(rays, cone, H, W, rows=None, cols=None):
    """(origins, directions), each [V, ..., 3]: the rays of detector pixels of the views ``rays`` [V,12] = {a, p00, pu, pv}, by
    the formula the kernels read them with (csrc/ray_sampling.hpp: pixel_ray).  Pixel (r, c) is the point
    P = (p00 + c pu) + r pv; ``cone``: start a, direction P - a; parallel beam: start P, direction a.  Plain torch in the
    dtype and on the device of ``rays``, one rounded operation per step in that order (float32 rays give the projector's own
    rays bit for bit), and differentiable in ``rays``.

    ``rows`` = ``cols`` = None: the whole detector, [V,H,W,3].  Otherwise two integer tensors of one shape [V, ...] or
    [1, ...]: view v takes the pixels (rows[v], cols[v]) (the same ones in every view when the leading size is 1), and the
    result is [V, ..., 3].  A random subset of K pixels per view is rows, cols [V,K]; scattered (view, r, c) triples are
    ``pixel_rays(rays[view], cone, H, W, r[:, None], c[:, None])``."""
    if not isinstance(rays, torch.Tensor) or rays.dim() != 2 or rays.shape[1] != 12 or not rays.is_floating_point():
        raise ValueError("rays must be a float tensor [V,12], got %s" % (tuple(getattr(rays, "shape", ())),))
    H, W, V = int(H), int(W), rays.shape[0]
    if H < 1 or W < 1:
        raise ValueError("the detector must have at least one pixel, got %d x %d" % (H, W))
    if (rows is None) != (cols is None):
        raise ValueError("rows and cols come together")
    if rows is None:
        r = torch.arange(H, device=rays.device)[None, :, None].expand(1, H, W)
        c = torch.arange(W, device=rays.device)[None, None, :].expand(1, H, W)
    else:
        r, c = torch.as_tensor(rows, device=rays.device), torch.as_tensor(cols, device=rays.device)
        if r.shape != c.shape or r.dim() < 1 or r.shape[0] not in (1, V) or r.is_floating_point() or c.is_floating_point():
            raise ValueError("rows and cols must be integer tensors of one shape [V, ...] or [1, ...] with V = %d, got %s and %s"
                             % (V, tuple(r.shape), tuple(c.shape)))
    par = rays.reshape((V,) + (1,) * (r.dim() - 1) + (12,))
    fr, fc = r.to(rays.dtype)[..., None], c.to(rays.dtype)[..., None]
    point = (par[..., 3:6] + fc * par[..., 6:9]) + fr * par[..., 9:12]
    a = par[..., 0:3].expand_as(point)
    if cone:
        return a, point - a
    return point, a


def curved_detector_rays(angles, DSO, DSD, dGamma, dV, nDetector, offDetector=(0.0, 0.0)):
    """(origins, directions), each [V,H,W,3] float64: the rays of a circular scan about the z axis with an equiangular
    cylindrical detector focused on the source (the third-generation CT detector), which no [V,12] describes.

    ``angles`` [V]; ``DSO`` / ``DSD`` the source-to-axis and source-to-detector distances (the cylinder's radius);
    ``dGamma`` the fan angle between neighbouring columns in radians, ``dV`` the row pitch; ``nDetector`` = (H, W);
    ``offDetector`` = (along the rows' direction, along the arc: a length, DSD times the angle it adds).  Every continuous
    argument is a scalar or a per-view tensor [V]; float64 torch inside, differentiable in each, like ``scan_rays``, whose
    frame this is: the source of view i at DSO (cos t, sin t, 0), eu = (-sin t, cos t, 0), ev = (0, 0, -1),
    en = (-cos t, -sin t, 0).  Pixel (r, c) sits at the fan angle g = (c + 1/2 - W / 2) dGamma + offDetector[1] / DSD and the
    height v = (r + 1/2 - H / 2) dV + offDetector[0]:
        pixel = source + DSD (cos g en + sin g eu) + v ev.
    origins = the source; directions = (pixel - source) / DSD, the scale ``scan_rays`` gives its cone rays, so that on the
    column with g = 0 the rays are those of the flat detector of the same row pitch."""
    H, W = int(nDetector[0]), int(nDetector[1])
    if H < 1 or W < 1:
        raise ValueError("the detector must have at least one pixel, got %d x %d" % (H, W))
    tensors = [x for x in (angles, DSO, DSD, dGamma, dV) if isinstance(x, torch.Tensor)]
    tensors += [x for x in ([offDetector] if isinstance(offDetector, torch.Tensor) else offDetector) if isinstance(x, torch.Tensor)]
    device = tensors[0].device if tensors else torch.device("cpu")
    ang = (angles.to(device=device, dtype=_F64) if isinstance(angles, torch.Tensor)
           else torch.as_tensor(angles, dtype=_F64, device=device)).reshape(-1)
    V = ang.shape[0]
    if V < 1:
        raise ValueError("no views")
    DSO, DSD, dGamma, dV = (_per_view(x, V, device)[:, None, None] for x in (DSO, DSD, dGamma, dV))
    oV, oU = (x[:, None, None] for x in _several(offDetector, 2, "offDetector", V, device))
    c, s = torch.cos(ang), torch.sin(ang)
    zero, one = torch.zeros_like(c), torch.ones_like(c)
    eu = torch.stack([-s, c, zero], 1)[:, None, None, :]
    ev = torch.stack([zero, zero, -one], 1)[:, None, None, :]
    en = torch.stack([-c, -s, zero], 1)[:, None, None, :]
    src = DSO[..., None] * torch.stack([c, s, zero], 1)[:, None, None, :]
    g = (torch.arange(W, dtype=_F64, device=device)[None, None, :] + (0.5 - 0.5 * W)) * dGamma + oU / DSD
    v = (torch.arange(H, dtype=_F64, device=device)[None, :, None] + (0.5 - 0.5 * H)) * dV + oV
    g, v = g.expand(V, H, W)[..., None], v.expand(V, H, W)[..., None]
    direction = torch.cos(g) * en + torch.sin(g) * eu + (v / DSD[..., None]) * ev
    return src.expand_as(direction), direction


def scanner_args(scanner, nDetector):
    """The keyword arguments of ``scan_rays`` that describe ``scanner`` (a config such as ``scene.CONE_BEAM``) on a detector
    of ``nDetector`` = (H, W) pixels, in world units: lengths times the scene scale 2 / max(sVoxel), as ``scene.make_view``
    scales them.  ``offDetector`` and ``offOrigin`` are the config's, which ``make_view`` ignores.  Parallel beam: the
    rasterizer's parallel detector spans the view-space square [-1, 1]^2 whatever sDetector says (projector.py), and so does
    this one."""
    scale = 2.0 / max(scanner["sVoxel"])
    H, W = int(nDetector[0]), int(nDetector[1])
    sDet = [s * scale for s in scanner["sDetector"]] if scanner["mode"] == "cone" else [2.0, 2.0]
    return dict(DSO=scanner["DSO"] * scale, DSD=scanner["DSD"] * scale, dDetector=(sDet[0] / H, sDet[1] / W), nDetector=(H, W),
                offDetector=tuple(o * scale for o in scanner.get("offDetector", (0.0, 0.0))),
                offOrigin=tuple(o * scale for o in scanner.get("offOrigin", (0.0, 0.0, 0.0))), mode=scanner["mode"])


ADAM_BETAS, ADAM_EPS = (0.9, 0.999), 1e-8


def refine_geometry(projs, cloud, rays_fn, params, iters, lr, loss="l2", cone=True, callback=None, rays_per_step=None, seed=0):
    """Geometric self-calibration: minimise the error of the cloud's exact projection against ``projs`` [V,H,W] (GPU) over
    the geometry, the cloud held fixed.

    ``cloud`` = (xyz, density, scaling, rotation), activated GPU tensors; ``params``: a dict of tensors, the starting values
    of the parameters to refine (copied; keep them on the cloud's device to avoid copies in the loop); ``rays_fn(params)``
    -> rays [V,12], differentiable torch code, typically ``scan_rays`` with some arguments taken from the dict.  Each of the
    ``iters`` steps projects exactly along rays_fn(params), takes ``loss`` ("l2": mean squared error, "l1": mean absolute
    error) and makes one step of torch.optim.Adam (betas 0.9 / 0.999, eps 1e-8, learning rate ``lr``) on the parameters.
    -> (refined parameters: a dict of detached tensors, loss history: a tensor [iters] on the device, the loss BEFORE each
    step).  Nothing in the loop waits for the device; ``callback(step, loss, params)``, when given, runs after every step and
    may.

    ``rays_per_step`` = None: every step projects the V whole views.  An integer K: every step draws K of the V * H * W pixels
    without replacement (``torch.randperm(V * H * W, generator=<CPU generator seeded once with seed>)[:K]``, then (view, row,
    col) by division), forms their rays with ``pixel_rays`` from the float32 rays_fn(params), integrates them with
    ``integrate_rays(..., half_line=cone, method="leaves")`` and takes the same loss over the K pixels.  The cloud is held
    fixed, so it is put into ``cloud_order`` once, before the loop.  With K = V * H * W every pixel appears once per step and
    the loss is the full loss up to the association of its sum.
    """
    from .gaussian_projector import cloud_order, integrate_rays, project_gaussians_rays
    if loss not in ("l2", "l1"):
        raise ValueError("loss must be 'l2' or 'l1', got %r" % (loss,))
    if not isinstance(projs, torch.Tensor) or projs.dim() != 3 or not projs.is_cuda:
        raise ValueError("projs must be a GPU tensor [V,H,W]")
    V, H, W = projs.shape
    if rays_per_step is not None and not 1 <= int(rays_per_step) <= V * H * W:
        raise ValueError("rays_per_step must lie in 1 .. V * H * W = %d, got %r" % (V * H * W, rays_per_step))
    cloud = tuple(t.detach() for t in cloud)
    p = {k: torch.as_tensor(v).detach().clone().requires_grad_(True) for k, v in params.items()}
    opt = torch.optim.Adam(list(p.values()), lr=lr, betas=ADAM_BETAS, eps=ADAM_EPS)
    history = torch.zeros((int(iters),), dtype=torch.float32, device=projs.device)
    target = projs.detach().to(torch.float32)
    gen = None
    if rays_per_step is not None:
        K, total = int(rays_per_step), V * H * W
        perm = cloud_order(cloud[0], cloud[2])
        cloud = tuple(t[perm].contiguous() for t in cloud)
        gen = torch.Generator(device="cpu").manual_seed(int(seed))
        flat = target.reshape(-1)
    for it in range(int(iters)):
        opt.zero_grad(set_to_none=True)
        if gen is None:
            diff = project_gaussians_rays(rays_fn(p), cone, H, W, *cloud) - target
        else:
            pick = torch.randperm(total, generator=gen)[:K].to(projs.device)
            view = pick // (H * W)
            rest = pick - view * (H * W)
            row = rest // W
            col = rest - row * W
            o, d = pixel_rays(rays_fn(p).to(device=projs.device, dtype=torch.float32)[view], cone, H, W, row[:, None], col[:, None])
            diff = integrate_rays(o, d, *cloud, half_line=cone, method="leaves").reshape(-1) - flat[pick]
        value = (diff * diff).mean() if loss == "l2" else diff.abs().mean()
        value.backward()
        opt.step()
        history[it] = value.detach()
        if callback is not None:
            callback(it, value.detach(), p)
    return {k: v.detach() for k, v in p.items()}, history


def ray_jacobian(rays, cone, H, W, xyz, density, scaling, rotation, scale_modifier=1.0, plan=None):
    """Every pixel's derivative in its own ray, [V,6,H,W] (GPU, float32): planes 0..2 hold d pixel / d s, planes 3..5
    d pixel / d d, for the start s and the direction d ``pixel_rays`` gives the pixel, of ``project_gaussians_rays`` on the
    same arguments (``r2_project_gaussians_ray_jacobian``: one launch, pixel-major, no workspace, no host synchronisation).
    Six numbers per pixel are the whole ray Jacobian: any number of geometry parameters chains through them in torch
    (``gaussian_projector.contract_ray_jacobian``), which is what ``refine_geometry_lm`` does.  Not differentiable.
    ``plan``: a ``gaussian_projector.ProjectionPlan`` built from these very tensors; the launch then walks its lists and gives
    the same bits.  (``refine_geometry`` and ``refine_geometry_lm`` move the rays every iteration and take no plan.)"""
    from .gaussian_projector import _ray_jacobian
    return _ray_jacobian(rays, cone, H, W, xyz, density, scaling, rotation, scale_modifier, plan)


def refine_geometry_lm(projs, cloud, rays_fn, params, iters, damping=1e-3, cone=True, weights=None, callback=None):
    """``refine_geometry`` by Levenberg-Marquardt: the same least-squares problem, solved with the Jacobian instead of the
    gradient, in a handful of steps where Adam takes tens.

    ``projs``, ``cloud``, ``rays_fn``, ``params`` and ``cone`` as in ``refine_geometry``; ``weights`` [V,H,W] (GPU, >= 0; None:
    1) are the pixels' inverse variances.  With k parameters in all, r the residual and J [V H W, k] its Jacobian, a step
    solves (J^T W J + damping diag(J^T W J)) delta = -J^T W r: Marquardt's scaling, assembled and solved in float64 on the
    device.  J comes from one ``ray_jacobian`` launch, whatever k is, contracted with d rays / d params, which
    ``torch.func.jacfwd`` takes of ``rays_fn`` in float64.  The step is accepted when the mean weighted squared error falls;
    ``damping`` is divided by 10 then and multiplied by 10 otherwise (the parameters stay, and the next iteration solves again
    with the Jacobian it has).  Per iteration: one forward launch, for the candidate, and at most one ``ray_jacobian`` launch;
    and ONE host read, of the comparison that decides the step.
    -> (refined parameters: a dict of detached tensors, loss history: a float64 tensor [iters] on the device, the loss BEFORE
    each step).  ``callback(step, loss, params)``, when given, runs after every step."""
    from .gaussian_projector import contract_ray_jacobian, project_gaussians_rays
    if not isinstance(projs, torch.Tensor) or projs.dim() != 3 or not projs.is_cuda:
        raise ValueError("projs must be a GPU tensor [V,H,W]")
    V, H, W = projs.shape
    dev = projs.device
    if weights is not None and (not isinstance(weights, torch.Tensor) or tuple(weights.shape) != (V, H, W) or weights.device != dev):
        raise ValueError("weights must be a tensor [%d,%d,%d] on %s, got %s" % (V, H, W, dev, tuple(getattr(weights, "shape", ()))))
    if not params:
        raise ValueError("no parameters to refine")
    if not float(damping) >= 0:
        raise ValueError("damping must be >= 0, got %r" % (damping,))
    cloud = tuple(t.detach() for t in cloud)
    start = {k: torch.as_tensor(v).detach() for k, v in params.items()}
    sizes = [v.numel() for v in start.values()]
    x = torch.cat([v.reshape(-1).to(device=dev, dtype=_F64) for v in start.values()])

    def unflatten(flat):
        parts = torch.split(flat, sizes)
        return {k: p.reshape(v.shape) for (k, v), p in zip(start.items(), parts)}

    def rays_of(flat):
        return rays_fn(unflatten(flat)).to(_F64)

    target = projs.detach().to(torch.float32)
    w = None if weights is None else weights.detach().to(_F64).reshape(-1)

    def residual(flat):
        r = (project_gaussians_rays(rays_of(flat).detach(), cone, H, W, *cloud) - target).to(_F64).reshape(-1)
        return r, ((r * r) if w is None else (w * r * r)).mean()

    lam = float(damping)
    res, loss = residual(x)
    history = torch.zeros((int(iters),), dtype=_F64, device=dev)
    fresh = True
    for it in range(int(iters)):
        history[it] = loss
        if fresh:
            jac = ray_jacobian(rays_of(x).detach(), cone, H, W, *cloud)
            dr = torch.func.jacfwd(rays_of)(x)                                                  # [V,12,k]
            J = torch.stack([contract_ray_jacobian(jac, dr[:, :, k], cone).reshape(-1) for k in range(x.numel())], 1)
            JW = J if w is None else J * w[:, None]
            A, g = JW.T @ J, JW.T @ res
        cand = x + torch.linalg.solve(A + lam * torch.diag(torch.diagonal(A)), -g)
        rc, lc = residual(cand)
        fresh = bool(lc < loss)   # the one host read of the iteration
        if fresh:
            x, res, loss, lam = cand, rc, lc, lam / 10.0
        else:
            lam = lam * 10.0
        if callback is not None:
            callback(it, history[it], unflatten(x))
    return {k: v.detach().to(start[k].dtype) if start[k].is_floating_point() else v.detach() for k, v in unflatten(x).items()}, history
