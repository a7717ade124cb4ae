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
from ._boundary import _F32, call as _call, f32c, ptr_table, require_gpu, workspace

NAMES = ("xyz", "density", "scaling", "rotation")
_WIDTHS = (3, 1, 3, 4)
MAX_ROWS = 1 << 29


def _u64(v, name):
    v = int(v)
    if not 0 <= v < 1 << 64:
        raise ValueError("%s must fit 64 unsigned bits, got %r" % (name, v))
    return C.c_ulonglong(v)


def _activated(P, dev, density, scaling, rotation):
    out = []
    for t, w, name in zip((density, scaling, rotation), (1, 3, 4), ("density", "scaling", "rotation")):
        require_gpu(t, name)
        if t.ndim == 1 and w == 1:
            t = t[:, None]
        if tuple(t.shape) != (P, w) or t.device != dev:
            raise ValueError("activated %s must be [%d, %d] on %s, got %s on %s" % (name, P, w, dev, tuple(t.shape), t.device))
        out.append(f32c(t.detach()))
    return out


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
    d, s, r = _activated(P, dev, density, scaling, rotation)
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
    ps = [f32c(params[n].detach()) for n in NAMES]
    for n, t, w in zip(NAMES, ps, _WIDTHS):
        if tuple(t.shape) != (P, w) or t.device != dev:
            raise ValueError("%s must be [%d, %d] on %s, got %s" % (n, P, w, dev, tuple(t.shape)))
    have_m = moments is not None
    ms = [f32c(moments[n][0]) for n in NAMES] if have_m else [None] * 4
    vs = [f32c(moments[n][1]) for n in NAMES] if have_m else [None] * 4
    for t, w in zip(ms + vs, _WIDTHS + _WIDTHS):
        if t is not None and (tuple(t.shape) != (P, w) or t.device != dev):
            raise ValueError("a moment array is %s, not [%d, %d] on %s" % (tuple(t.shape), P, w, dev))
    st = None
    if stats is not None:
        st = [f32c(t.detach()).reshape(-1) for t in stats]
        if len(st) != 3 or any(t.numel() != P or t.device != dev for t in st):
            raise ValueError("stats must be (max_radii2D, grad_accum, denom) with %d elements each" % P)
    if weights is not None:
        require_gpu(weights, "weights")
        weights = f32c(weights.detach()).reshape(-1)
        if weights.numel() != P or weights.device != dev:
            raise ValueError("weights must have %d elements on %s" % (P, dev))
    if activated is None:
        from .gaussians import activate
        activated = activate(ps[1], ps[2], ps[3], scale_bound) if P else tuple(
            torch.empty((0, w), dtype=_F32, device=dev) for w in (1, 3, 4))
    act = _activated(P, dev, *activated)
    Pn = P + n_new
    po = [torch.empty((Pn, w), dtype=_F32, device=dev) for w in _WIDTHS]
    mo = [torch.empty((Pn, w), dtype=_F32, device=dev) if have_m else None for w in _WIDTHS]
    vo = [torch.empty((Pn, w), dtype=_F32, device=dev) if have_m else None for w in _WIDTHS]
    so = [torch.empty((Pn,), dtype=_F32, device=dev) for _ in range(3)] if st is not None else [None] * 3
    sources = torch.empty((Pn,), dtype=torch.int32, device=dev)     # both written in full by r2_relocate_plan
    draws = torch.empty((P,), dtype=torch.int32, device=dev)
    info = dict(P=Pn, sources=sources, draws=draws)
    if P:
        nbytes = int(_lib.lib().r2_relocate_workspace_bytes(P, n_new))
        ws = workspace(nbytes, dev)
        host = (C.c_uint * 3)() if counts else None
        sd, cl = _u64(seed, "seed"), _u64(call, "call")
        _call("r2_relocate_plan", dev, P, n_new, ptr_table(ps), act[0], weights, float(dead_density), sd, cl, sources, draws, ws,
              nbytes, host)
        _call("r2_relocate_emit", dev, P, n_new, ptr_table(ps), ptr_table(ms) if have_m else None,
              ptr_table(vs) if have_m else None, act[0], act[1], act[2], *(st if st is not None else [None] * 3), spread, sd, cl,
              sources, draws, ws, nbytes, ptr_table(po), ptr_table(mo) if have_m else None, ptr_table(vo) if have_m else None,
              *so)
        if counts:
            info.update(dead=int(host[0]), alive=int(host[1]), drawable=int(host[2]))
    elif counts:
        info.update(dead=0, alive=0, drawable=0)
    new_params = dict(zip(NAMES, po))
    new_moments = {n: (m, v) for n, m, v in zip(NAMES, mo, vo)} if have_m else None
    return new_params, new_moments, (tuple(so) if st is not None else None), info


__all__ = ["position_noise", "relocate"]
