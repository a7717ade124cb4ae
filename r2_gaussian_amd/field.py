"""Exact evaluation of the Gaussian model's density field at caller-supplied points,
``sigma(x) = sum_i rho_i exp(-(x - mu_i)^T Sigma_i^-1 (x - mu_i) / 2)``, on the kernels of csrc/gaussian_query.hip and
csrc/gaussian_query_bwd.hip (``r2_query_gaussians`` and its backward; include/r2hip.h states the contract).

The voxelizer is the reference's approximation of this field on one axis-aligned grid: every Gaussian cut at a cube of
ceil(3 max(scale) / dVoxel) voxels and at alpha >= 1e-6.  Here a pair is only skipped when its exponent q exceeds 32 (below
exp(-16) of the Gaussian's peak), the points are the caller's (an oblique plane, a line profile finer than the grid, a patch,
scattered samples), and the operator is differentiable in the points as well as in the four parameter tensors.
"""
import torch

from . import _lib
from ._boundary import _F32, call, cloud, f32c, require_gpu, workspace


def _spread10(v):
    """The low 10 bits of an int64 tensor, two zero bits after each."""
    v = (v | (v << 16)) & 0x030000FF
    v = (v | (v << 8)) & 0x0300F00F
    v = (v | (v << 4)) & 0x030C30C3
    return (v | (v << 2)) & 0x09249249


def morton_order(points):
    """Permutation [N] (int64) that orders ``points`` [N,3] by the 30-bit Morton key of their position in their own bounding
    box (10 bits per axis, x in the lowest bit), by a stable sort: equal keys keep their order.  Points with a non-finite
    coordinate stay out of the box and get key 0.  torch ops only, on the points' device."""
    p = points.detach().to(torch.float64)
    finite = torch.isfinite(p).all(1, keepdim=True)
    if p.shape[0] == 0:
        return torch.arange(0, device=p.device)
    big = torch.finfo(torch.float64).max
    lo = torch.where(finite, p, torch.full_like(p, big)).amin(0)
    hi = torch.where(finite, p, torch.full_like(p, -big)).amax(0)
    ext = hi - lo
    cell = torch.where(ext > 0, (p - lo) / torch.where(ext > 0, ext, torch.ones_like(ext)) * 1024.0, torch.zeros_like(p))
    cell = torch.where(finite, cell, torch.zeros_like(cell)).floor().clamp_(0, 1023).to(torch.int64)
    key = _spread10(cell[:, 0]) | (_spread10(cell[:, 1]) << 1) | (_spread10(cell[:, 2]) << 2)
    return torch.sort(key, stable=True)[1]


def inverse_permutation(perm):
    inv = torch.empty_like(perm)
    inv[perm] = torch.arange(perm.shape[0], device=perm.device)
    return inv


class _QueryPoints(torch.autograd.Function):
    """points [N,3] -> [N].  ``perm`` (or None): the order the kernels see the points in; values and gradients come back in
    the caller's order, by gathers alone."""

    @staticmethod
    def forward(ctx, points, xyz, density, scaling, rotation, scale_modifier, perm):
        N, P = points.shape[0], xyz.shape[0]
        x, d, s, r = cloud(xyz, density, scaling, rotation)
        pts = f32c(points.detach())
        inv = None
        if perm is not None:
            pts, inv = pts[perm].contiguous(), inverse_permutation(perm)
        out = torch.empty((N,), dtype=_F32, device=x.device)
        call("r2_query_gaussians", x.device, N, pts, P, x, d, s, float(scale_modifier), r, out)
        ctx.save_for_backward(pts, x, d, s, r, perm, inv)
        ctx.mod = float(scale_modifier)
        return out if inv is None else out[inv]

    @staticmethod
    def backward(ctx, G):
        pts, x, d, s, r, perm, inv = ctx.saved_tensors
        N, P = pts.shape[0], x.shape[0]
        G = f32c(G)
        if perm is not None:
            G = G[perm].contiguous()
        gx, gd, gs, gr = torch.empty_like(x), torch.empty_like(d), torch.empty_like(s), torch.empty_like(r)
        gp = torch.empty_like(pts) if ctx.needs_input_grad[0] else None
        ws = workspace(_lib.lib().r2_query_gaussians_workspace_bytes(N), x.device, at_least=1)
        call("r2_query_gaussians_backward", x.device, N, pts, P, x, d, s, ctx.mod, r, G, gx, gd, gs, gr, gp, ws, ws.numel())
        if gp is not None and inv is not None:
            gp = gp[inv]
        return gp, gx, gd, gs, gr, None, None


def _check_cloud(xyz, density, scaling, rotation):
    for name, t, cols in (("xyz", xyz, 3), ("scaling", scaling, 3), ("rotation", rotation, 4)):
        if not isinstance(t, torch.Tensor) or t.dim() != 2 or t.shape[1] != cols:
            raise ValueError("%s must be a tensor [P,%d], got %s" % (name, cols, tuple(getattr(t, "shape", ()))))
    P = xyz.shape[0]
    if not isinstance(density, torch.Tensor) or tuple(density.shape) not in ((P, 1), (P,)):
        raise ValueError("density must be a tensor [P,1] or [P] with P = %d, got %s" % (P, tuple(getattr(density, "shape", ()))))
    if scaling.shape[0] != P or rotation.shape[0] != P:
        raise ValueError("xyz, scaling and rotation differ in P: %d, %d, %d" % (P, scaling.shape[0], rotation.shape[0]))
    for name, t in (("xyz", xyz), ("density", density), ("scaling", scaling), ("rotation", rotation)):
        require_gpu(t, name)
        if t.device != xyz.device:
            raise ValueError("%s is on %s, xyz on %s" % (name, t.device, xyz.device))
    if P > (1 << 29):
        raise ValueError("at most 2^29 Gaussians, got %d" % P)


def query_points(points, xyz, density, scaling, rotation, scale_modifier=1.0, sort=False):
    """The field at ``points`` [..., 3] -> [...] (GPU, float32), for the cloud ``xyz`` [P,3], ``density`` [P,1] or [P],
    ``scaling`` [P,3], ``rotation`` [P,4] (activated values; the quaternion is used as it comes).  Differentiable in the four
    parameter tensors, and in ``points`` when they require grad.  No host synchronisation.

    The kernels cull by blocks of 256 consecutive points: a block tests every Gaussian's bounding sphere against the box of
    its points.  Coherent inputs -- planes, lines, patches, voxel grids in their natural order -- cull well as they are.
    ``sort=True`` is meant for scattered point sets: it orders the points by a 30-bit Morton key of their position in their
    own bounding box (``morton_order``: torch ops, a stable sort) before the kernels see them and un-permutes the values
    and the gradients; the result is the same."""
    if not isinstance(points, torch.Tensor) or points.dim() < 1 or points.shape[-1] != 3:
        raise ValueError("points must be a tensor [..., 3], got %s" % (tuple(getattr(points, "shape", ())),))
    require_gpu(points, "points")
    _check_cloud(xyz, density, scaling, rotation)
    if points.device != xyz.device:
        raise ValueError("points are on %s, xyz on %s" % (points.device, xyz.device))
    flat = points.reshape(-1, 3)
    if flat.shape[0] >= (1 << 31):
        raise ValueError("fewer than 2^31 points, got %d" % flat.shape[0])
    perm = morton_order(flat) if sort else None
    return _QueryPoints.apply(flat, xyz, density, scaling, rotation, float(scale_modifier), perm).reshape(points.shape[:-1])


def plane_points(origin, du, dv, H, W, device):
    """[H,W,3] float32 on ``device``: the lattice origin + c du + r dv (r the row, c the column), each coordinate computed as
    (origin + c du) + r dv in float32."""
    H, W = int(H), int(W)
    if H < 1 or W < 1:
        raise ValueError("the plane must have at least one point, got %d x %d" % (H, W))
    o, u, v = (torch.as_tensor(a, dtype=_F32).reshape(3).to(device) for a in (origin, du, dv))
    c = torch.arange(W, dtype=_F32, device=device)[None, :, None]
    r = torch.arange(H, dtype=_F32, device=device)[:, None, None]
    return (o + c * u) + r * v


def query_plane(origin, du, dv, H, W, xyz, density, scaling, rotation, scale_modifier=1.0):
    """The field [H,W] on the lattice origin + c du + r dv (``plane_points``): the oblique slice.  origin, du, dv: three
    world coordinates each."""
    if not isinstance(xyz, torch.Tensor):
        raise ValueError("xyz must be a tensor [P,3]")
    require_gpu(xyz, "xyz")
    return query_points(plane_points(origin, du, dv, H, W, xyz.device), xyz, density, scaling, rotation, scale_modifier)


def voxel_centres(center, nVoxel, sVoxel, device=None):
    """[nx,ny,nz,3] float32: the world positions the voxelizer samples.  Voxel idx sits at
    center - sVoxel / 2 + (idx + 0.5) sVoxel / nVoxel (computed in float64, rounded once)."""
    if len(center) != 3 or len(nVoxel) != 3 or len(sVoxel) != 3 or not all(int(n) > 0 for n in nVoxel):
        raise ValueError("center, nVoxel and sVoxel must have three entries each, nVoxel positive")
    ax = [float(c) - float(s) / 2 + (torch.arange(int(n), dtype=torch.float64) + 0.5) * (float(s) / int(n))
          for c, n, s in zip(center, nVoxel, sVoxel)]
    grid = torch.stack(torch.meshgrid(*ax, indexing="ij"), -1).to(_F32)
    return grid if device is None else grid.to(device)
