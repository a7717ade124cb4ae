"""A fixed budget of Gaussians: covariance-shaped position noise and the relocation of dead Gaussians onto live ones
(include/r2hip.h: r2_gaussian_noise, r2_relocate_plan, r2_relocate_emit; csrc/gaussian_mcmc.hip).  The strategy of "3D Gaussian
Splatting as Markov Chain Monte Carlo" (Kheradmand et al. 2024); no counterpart in the reference, whose density control is the
threshold clone / split / prune of densify.py.

    position_noise(xyz, density, scaling, rotation, lr, call=it)                    # in place on the raw xyz
    params, moments, stats, info = relocate(params, moments, stats, 0.005, n_new=k, call=it, activated=(d, s, r))

The field here is a plain sum, so n + 1 copies of a Gaussian with density rho / (n + 1) each are that Gaussian: relocation with
spread = 0 leaves ``field.query_points`` and ``gaussian_projector.project_gaussians`` unchanged.  Randomness is counter-based
(csrc/philox.hpp): a result is a function of (seed, call) and the inputs, and of nothing else.  Nothing here is differentiated,
and nothing reads the device unless ``counts=True``.

The defaults (noise_lr 5e5, density 0.005, sharpness 0.5, dead_density 0.005) are the original method's numbers for opacities of
a colour scene; nobody has tuned them for CT densities yet.
"""
import ctypes as C

import torch

from . import _lib
from ._boundary import _F32, NAMES, WIDTHS, call as _call, cloud_checked, f32c, require_gpu, rows_emit, rows_in, workspace

MAX_ROWS = 1 << 29


def _u64(v, name):
    v = int(v)
    if not 0 <= v < 1 << 64:
        raise ValueError("%s must fit 64 unsigned bits, got %r" % (name, v))
    return C.c_ulonglong(v)


def position_noise(xyz, density, scaling, rotation, lr, density_threshold=0.005, sharpness=0.5, seed=0, call=0):
    """xyz += lr * gate * R S^2 R^T eps, IN PLACE on the raw xyz [P, 3] (contiguous float32); density [P, 1], scaling [P, 3] and
    rotation [P, 4] are ACTIVATED.  eps ~ N(0, 1) from (seed, call, row); gate = 1 / (1 + exp(sharpness (density /
    density_threshold - 1))): near 1 for a Gaussian that has faded, 0 for one that carries density.  lr: the xyz learning rate
    times the noise scale.  A row with a non-finite density, scale or quaternion is left untouched.  One launch, no host read.
    -> xyz."""
    require_gpu(xyz, "xyz")
    if xyz.ndim != 2 or xyz.shape[1] != 3 or xyz.dtype != _F32 or not xyz.is_contiguous():
        raise ValueError("xyz must be a contiguous float32 [P, 3] tensor (it is updated in place), got %s %s" % (
            tuple(xyz.shape), xyz.dtype))
    P, dev = xyz.shape[0], xyz.device
    d, s, r = cloud_checked((density, scaling, rotation), P, dev, NAMES[1:])
    if P:
        _call("r2_gaussian_noise", dev, P, xyz.detach(), d, s, r, float(lr), float(density_threshold), float(sharpness),
              _u64(seed, "seed"), _u64(call, "call"))
    return xyz


def relocate(params, moments, stats, dead_density, n_new=0, weights=None, spread=0.0, seed=0, call=0, counts=False,
             activated=None, scale_bound=None):
    """Move every dead row onto a live one and append n_new rows, P + n_new rows in all.

    params: dict name -> RAW parameter ([P,3], [P,1], [P,3], [P,4]); moments: dict name -> (exp_avg, exp_avg_sq), or None;
    stats: (max_radii2D, grad_accum, denom) with P elements each, or None; activated: (density, scaling, rotation) of these raw
    parameters (GaussianModel's ``_act``), computed here under ``scale_bound`` when None.
    A row is dead when its activated density is not inside (dead_density, +inf) or a raw parameter is not finite.  Every dead
    row and every appended row (a "slot") draws a source among the alive rows in proportion to ``weights`` [P] (None: the
    activated density; rows whose weight is not finite and > 0 are never drawn), slot k with the generator's words of
    (seed, call, k).  A source drawn n times and its n slots all get the density rho / (n + 1), and zero Adam moments and
    statistics; the slots copy the source's xyz, scaling and rotation bit for bit -- displaced by spread * R S eps with
    spread > 0 -- and every other row is carried over bit for bit.  With nothing to draw from, the rows are copied and the
    appended ones are parked as dead copies (raw density -100) for the next call.
    -> (params, moments, stats, info): info = dict(P = P + n_new, sources [P + n_new] int32: slot k's source or -1,
    draws [P] int32: n per row) and, with counts=True (one host read), dead / alive / drawable."""
    xyz = params["xyz"]
    require_gpu(xyz, "xyz")
    dev, P = xyz.device, int(xyz.shape[0])
    n_new = int(n_new)
    if n_new < 0 or P + n_new > MAX_ROWS or (P == 0 and n_new > 0):
        raise ValueError("n_new must be >= 0, P + n_new <= 2^29 and P > 0 to append, got P = %d, n_new = %d" % (P, n_new))
    spread = float(spread)
    if not 0.0 <= spread < float("inf"):
        raise ValueError("spread must be in [0, inf), got %r" % (spread,))
    rows = rows_in(params, moments, stats, P, dev)
    ps, st = rows[0], rows[3]
    if weights is not None:
        require_gpu(weights, "weights")
        weights = f32c(weights.detach()).reshape(-1)
        if weights.numel() != P or weights.device != dev:
            raise ValueError("weights must have %d elements on %s" % (P, dev))
    if activated is None:
        from .gaussians import activate
        activated = activate(ps[1], ps[2], ps[3], scale_bound) if P else tuple(
            torch.empty((0, WIDTHS[n]), dtype=_F32, device=dev) for n in NAMES[1:])
    act = cloud_checked(activated, P, dev, NAMES[1:])
    Pn = P + n_new
    sources = torch.empty((Pn,), dtype=torch.int32, device=dev)     # both written in full by r2_relocate_plan
    draws = torch.empty((P,), dtype=torch.int32, device=dev)
    info = dict(P=Pn, sources=sources, draws=draws)
    host = (C.c_uint * 3)() if counts else None

    def emit(tin, tout, so):
        if not P:
            return
        nbytes = int(_lib.lib().r2_relocate_workspace_bytes(P, n_new))
        ws = workspace(nbytes, dev)
        sd, cl = _u64(seed, "seed"), _u64(call, "call")
        _call("r2_relocate_plan", dev, P, n_new, tin[0], act[0], weights, float(dead_density), sd, cl, sources, draws, ws, nbytes, host)
        _call("r2_relocate_emit", dev, P, n_new, *tin, *act, *(st if st is not None else [None] * 3), spread, sd, cl, sources, draws,
              ws, nbytes, *tout, *so)

    new_params, new_moments, new_stats = rows_emit(Pn, dev, rows, emit)
    if counts:
        info.update(dead=int(host[0]), alive=int(host[1]), drawable=int(host[2]))
    return new_params, new_moments, new_stats, info


__all__ = ["position_noise", "relocate"]
