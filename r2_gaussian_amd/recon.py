"""Classical iterative CT reconstructions without TIGRE: CGLS, SART, OS-SART, ASD-POCS and OS-ASD-POCS, the baselines of
the reference's ``run_ct_recon_algs`` (r2_gaussian/utils/ct_utils.py:60-215) and ``scripts/run_traditional_methods.py``.

They stand on two MI355X kernels behind the C ABI: the forward projector ``r2_project_volume`` (``A``) and its exact
transpose ``r2_backproject_volume`` (``A^T``, csrc/backprojector.hip), plus ``r2_tv_descent`` (csrc/tv_descent.hip) for the TV
steps of ASD-POCS.  ``projection_type="siddon"`` swaps the pair for the ray-voxel intersection model,
``r2_project_volume_siddon`` and its exact transpose ``r2_backproject_volume_siddon`` (csrc/backprojector_siddon.hip); the
default everywhere is ``"interpolated"``.  Both directions live in projector.py: ``Operator``, ``backproject`` and
``backproject_views`` are its names, imported here for the callers that know them as this module's.  The vector updates between them are elementwise tensor operations; every data-dependent scalar
stays a 0-d device tensor, so an iteration makes no host synchronisation unless ``computel2`` or ``verbose`` asks for one.

Conventions are those of ``projector.project`` and ``fdk.fdk``: the raw scanner config and its length units, projections
[V, H, W] as datagen writes them (rasterizer row order), volumes [nx, ny, nz] in ``query()`` layout.  In those units the
operator is ``A = project(., angles, cfg)``, i.e. ``A_scene / scale`` with ``scale = 2 / max(sVoxel)``, and
``backproject`` is its transpose ``A_scene^T / scale``.

The algorithms are restated from their published definitions (INTEGRATION.md lists where they knowingly differ from TIGRE):

* CGLS (Hestenes-Stiefel / Bjorck): x0 = 0, r = b, p = s = A^T r, gamma = |s|^2; per iteration q = A p,
  alpha = gamma / |q|^2, x += alpha p, r -= alpha q, s = A^T r, gamma' = |s|^2, p = s + (gamma' / gamma) p.
* OS-SART (Jiang & Wang; SART is blocksize 1): W = 1 / (A 1) per ray (0 where a ray misses), V_B = A_B^T 1 per block of
  consecutive views in input order (V^-1 = 0 where V_B = 0); for each block x <- max(0, x + lambda V_B^-1 (A_B^T (W (b_B -
  A_B x)))), and lambda <- lambda lambda_red after each sweep over all blocks.
* ASD-POCS (Sidky & Pan 2008), see ``os_asd_pocs``.
* FISTA-TV (Beck & Teboulle 2009), see ``fista_tv``: the one method here whose result is defined by an objective,
  1/2 |A x - b|^2 + lambda TV(x) over x >= 0, on the proximal operator of TV ``tv_prox`` (``r2_tv_prox``, csrc/tv_prox.hip).
"""
import argparse
import json
import os
import os.path as osp
import time

import numpy as np
import torch

from . import _lib
from . import fdk as F
from . import projector as P
from ._boundary import _F32, call, require_gpu
from .projector import Operator, _projections, backproject, backproject_views   # noqa: F401
_F64 = torch.float64
METHODS = ("fdk", "sart", "ossart", "asd_pocs", "os_asd_pocs", "cgls", "fista_tv")


def _sq(t):
    return t.pow(2).sum(dtype=_F64)


# ---- CGLS -----------------------------------------------------------------------------------------------------------------

def cgls(projs, angles, cfg, niter=60, computel2=False, accuracy=None, device="cuda", projection_type="interpolated"):
    """CGLS from x0 = 0: ``niter`` iterations on |A x - b|_2.  -> x [nx,ny,nz] (GPU), or (x, l2) with computel2, l2 the
    residual norms |b - A x_k| after each iteration (a host list: one synchronisation per iteration)."""
    op = Operator(angles, cfg, accuracy, device, projection_type)
    b = _projections(projs, op)
    if int(niter) < 0:
        raise ValueError("niter must be >= 0")
    x = torch.zeros(op.nVoxel, dtype=_F32, device=op.device)
    r = b.clone()
    p = op.At(r)
    s = torch.empty_like(p)
    q = torch.empty_like(b)
    gamma = _sq(p)
    zero = torch.zeros((), dtype=_F64, device=op.device)
    l2 = []
    for _ in range(int(niter)):
        op.A(p, out=q)
        qq = _sq(q)
        alpha = torch.where(qq > 0, gamma / torch.where(qq > 0, qq, 1.0), zero).to(_F32)
        x.add_(p * alpha)
        r.sub_(q * alpha)
        if computel2:
            l2.append(float(torch.linalg.vector_norm(r, dtype=_F64)))
        op.At(r, out=s)
        gamma_new = _sq(s)
        beta = torch.where(gamma > 0, gamma_new / torch.where(gamma > 0, gamma, 1.0), zero).to(_F32)
        p = s + beta * p
        gamma = gamma_new
    return (x, l2) if computel2 else x


# ---- SART / OS-SART ---------------------------------------------------------------------------------------------------------

class _Sart:
    """The weights of OS-SART for one operator and block size, computed once: W = 1/(A 1) per ray, V_B^-1 per block."""

    def __init__(self, op, blocksize):
        if int(blocksize) < 1:
            raise ValueError("blocksize must be >= 1, got %r" % (blocksize,))
        self.op = op
        bs = int(blocksize)
        self.blocks = [(v0, min(v0 + bs, op.V)) for v0 in range(0, op.V, bs)]
        ones = torch.ones(op.nVoxel, dtype=_F32, device=op.device)
        a1 = op.A(ones)
        self.W = torch.where(a1 > 0, 1.0 / torch.where(a1 > 0, a1, 1.0), torch.zeros_like(a1))
        one_p = torch.ones((op.V, op.H, op.W), dtype=_F32, device=op.device)
        self.Vinv = []
        for v0, v1 in self.blocks:
            v = op.At(one_p[v0:v1], v0, v1)
            self.Vinv.append(torch.where(v > 0, 1.0 / torch.where(v > 0, v, 1.0), torch.zeros_like(v)))

    def sweep(self, x, b, lmbda, nonneg=True):
        """One pass over all blocks, in place."""
        op = self.op
        for (v0, v1), vinv in zip(self.blocks, self.Vinv):
            res = op.A(x, v0, v1)
            res = (b[v0:v1] - res).mul_(self.W[v0:v1])
            upd = op.At(res, v0, v1)
            x.addcmul_(upd, vinv, value=float(lmbda))
            if nonneg:
                x.clamp_(min=0.0)
        return x


def ossart(projs, angles, cfg, niter=20, blocksize=10, lmbda=1.0, lmbda_red=0.999, init=None, nonneg=True, computel2=False,
           accuracy=None, device="cuda", projection_type="interpolated"):
    """OS-SART: ``niter`` sweeps over blocks of ``blocksize`` consecutive views (input order).  -> x (GPU), or (x, l2) with
    computel2 (|A x - b|_2 after each sweep; one synchronisation per sweep)."""
    op = Operator(angles, cfg, accuracy, device, projection_type)
    b = _projections(projs, op)
    st = _Sart(op, blocksize)
    x = _init(init, op)
    lam = float(lmbda)
    l2 = []
    for _ in range(int(niter)):
        st.sweep(x, b, lam, nonneg)
        lam *= lmbda_red
        if computel2:
            l2.append(float(torch.linalg.vector_norm(op.A(x) - b, dtype=_F64)))
    return (x, l2) if computel2 else x


def sart(projs, angles, cfg, niter=20, lmbda=1.0, lmbda_red=0.999, init=None, nonneg=True, computel2=False, accuracy=None,
         device="cuda", projection_type="interpolated"):
    """SART: OS-SART with one view per block."""
    return ossart(projs, angles, cfg, niter, 1, lmbda, lmbda_red, init, nonneg, computel2, accuracy, device,
                  projection_type)


def _init(init, op):
    if init is None:
        return torch.zeros(op.nVoxel, dtype=_F32, device=op.device)
    x = torch.as_tensor(init).to(device=op.device, dtype=_F32).clone().contiguous()
    if tuple(x.shape) != op.nVoxel:
        raise ValueError("init must be [%d,%d,%d]" % op.nVoxel)
    return x


# ---- TV descent and ASD-POCS ------------------------------------------------------------------------------------------------

def tv_descent(vol, step, n_iter, scratch=None):
    """``n_iter`` steps x <- x - step g / |g|_2, g = grad TV_eps(x) (include/r2hip.h, r2_tv_descent), in place on ``vol``
    [nx,ny,nz] (contiguous float32, GPU).  ``step``: a float or a 0-d device tensor (read on the device).  -> vol."""
    require_gpu(vol, "vol")
    if vol.dim() != 3 or vol.dtype != _F32 or not vol.is_contiguous():
        raise ValueError("vol must be a contiguous float32 [nx,ny,nz] tensor")
    if int(n_iter) < 0:
        raise ValueError("n_iter must be >= 0")
    if isinstance(step, torch.Tensor):
        st = step.to(device=vol.device, dtype=_F32).reshape(())
    else:
        st = torch.full((), float(step), dtype=_F32, device=vol.device)
    nx, ny, nz = vol.shape
    nbytes = int(_lib.lib().r2_tv_descent_scratch_bytes(nx, ny, nz))
    if scratch is None or scratch.numel() * scratch.element_size() < nbytes or scratch.device != vol.device:
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=vol.device)
    call("r2_tv_descent", vol.device, nx, ny, nz, vol, st, int(n_iter), scratch, scratch.numel() * scratch.element_size())
    return vol


def maxl2err_default(projs, angles, cfg, device="cuda", projection_type="interpolated"):
    """The reference's ASD-POCS tolerance: 0.15 |A fdk(b) - b|_2 (a 0-d device tensor)."""
    op = Operator(angles, cfg, None, device, projection_type)
    b = _projections(projs, op)
    return 0.15 * torch.linalg.vector_norm(op.A(F.fdk(b, angles, cfg, device=device)) - b, dtype=_F64)


def os_asd_pocs(projs, angles, cfg, niter=10, blocksize=10, tviter=20, maxl2err=None, alpha=0.002, lmbda=1.0,
                lmbda_red=0.9999, alpha_red=0.95, rmax=0.94, init=None, verbose=False, accuracy=None, device="cuda",
                return_trace=False, projection_type="interpolated"):
    """OS-ASD-POCS (Sidky & Pan 2008, with OS-SART as the data step; ASD-POCS is blocksize 1).  Each iteration:

    1. x_prev = x; one (OS-)SART sweep with the current lambda, clipped to x >= 0; x_sart = x.
    2. dd = |A x_sart - b|_2, dp = |x_sart - x_prev|_2; on the first iteration dtvg = alpha dp.
    3. ``tviter`` TV descent steps of length dtvg (``tv_descent``).
    4. dg = |x - x_sart|_2; if dg > rmax dp and dd > maxl2err: dtvg <- dtvg alpha_red.
    5. lambda <- lambda lambda_red.
    6. c = <x - x_sart, x_sart - x_prev> / max(dg dp, 1e-6); stop when c < -0.99 and dd <= maxl2err, or after ``niter``.

    ``maxl2err`` None: 0.15 |A fdk(b) - b|_2.  The stop test is kept on the device: once it holds, later iterations leave x
    as it is, so no iteration waits for the host unless ``verbose``.  -> x (GPU); with return_trace also a dict of per-
    iteration device tensors (dd, dp, dg, dtvg, reduced, c, active, sart_min = min x_sart)."""
    op = Operator(angles, cfg, accuracy, device, projection_type)
    b = _projections(projs, op)
    st = _Sart(op, blocksize)
    if maxl2err is None:
        maxl2err = maxl2err_default(b, angles, cfg, device, projection_type)
    eps = (maxl2err.to(device=op.device, dtype=_F64) if isinstance(maxl2err, torch.Tensor)
           else torch.full((), float(maxl2err), dtype=_F64, device=op.device))
    x = _init(init, op)
    lam = float(lmbda)
    active = torch.ones((), dtype=torch.bool, device=op.device)
    dtvg = torch.zeros((), dtype=_F32, device=op.device)
    scratch = torch.empty(int(_lib.lib().r2_tv_descent_scratch_bytes(*op.nVoxel)), dtype=torch.uint8, device=op.device)
    trace = {k: [] for k in ("dd", "dp", "dg", "dtvg", "reduced", "c", "active", "sart_min")}
    for it in range(int(niter)):
        x_prev = x.clone()
        st.sweep(x, b, lam, True)
        x_sart = x.clone()
        dd = torch.linalg.vector_norm(op.A(x_sart) - b, dtype=_F64)
        dp = torch.linalg.vector_norm(x_sart - x_prev, dtype=_F64)
        if it == 0:
            dtvg = (alpha * dp).to(_F32)
        tv_descent(x, dtvg, tviter, scratch)
        dg = torch.linalg.vector_norm(x - x_sart, dtype=_F64)
        reduced = (dg > rmax * dp) & (dd > eps)
        dtvg = torch.where(reduced, dtvg * alpha_red, dtvg)
        lam *= lmbda_red
        c = ((x - x_sart).double() * (x_sart - x_prev).double()).sum() / torch.clamp(dg * dp, min=1e-6)
        # a stopped run keeps the x it stopped with
        x.copy_(torch.where(active, x, x_prev))
        for k, v in (("dd", dd), ("dp", dp), ("dg", dg), ("dtvg", dtvg), ("reduced", reduced), ("c", c), ("active", active),
                     ("sart_min", x_sart.min())):
            trace[k].append(v)
        active = active & ~((c < -0.99) & (dd <= eps))
        if verbose:
            print("asd_pocs it %d: dd %.4g dp %.4g dg %.4g dtvg %.4g c %.4f" % (it, float(dd), float(dp), float(dg),
                                                                               float(dtvg), float(c)))
    return (x, trace) if return_trace else x


def asd_pocs(projs, angles, cfg, niter=10, tviter=20, maxl2err=None, alpha=0.002, lmbda=1.0, lmbda_red=0.9999,
             alpha_red=0.95, rmax=0.94, init=None, verbose=False, accuracy=None, device="cuda", return_trace=False,
             projection_type="interpolated"):
    """ASD-POCS: ``os_asd_pocs`` with one view per block (SART as the data step)."""
    return os_asd_pocs(projs, angles, cfg, niter, 1, tviter, maxl2err, alpha, lmbda, lmbda_red, alpha_red, rmax, init,
                       verbose, accuracy, device, return_trace, projection_type)


# ---- the TV proximal operator and FISTA-TV ----------------------------------------------------------------------------------

# Defaults of fista_tv, chosen by the sweep recorded in DESIGN.md section 4 ("TV proximal operator and FISTA-TV"): 64^3
# phantom, 20 noisy cone views of 96^2, PSNR against the phantom over a decade grid of lam.  The PSNR peaks at 1e-2 and does
# not depend on tviter between 10 and 50 (within 0.03 dB).
FISTA_LAM_REL = 1e-2
FISTA_TVITER = 20


def _scalar32(v, device):
    if isinstance(v, torch.Tensor):
        return v.to(device=device, dtype=_F32).reshape(())
    return torch.full((), float(v), dtype=_F32, device=device)


def tv_prox(vol, lam, n_iter=50, lo=None, hi=None, out=None, scratch=None):
    """argmin_x 1/2 |x - vol|^2 + lam TV(x) subject to lo <= x <= hi, by ``n_iter`` iterations of the fast gradient projection
    on the dual (include/r2hip.h, r2_tv_prox): TV is isotropic and unsmoothed, on the forward differences of ``tv_descent``.
    ``vol`` [nx,ny,nz]: contiguous float32 on the GPU, left as it is unless ``out`` is ``vol``.  ``lam``: a float or a 0-d
    device tensor (read on the device; <= 0 or NaN: the result is the clamp of ``vol``).  ``lo`` / ``hi``: floats, None for no
    bound.  ``out``: the result's tensor (like ``vol``; may be ``vol`` itself), ``scratch``: a GPU byte buffer of at least
    ``r2_tv_prox_scratch_bytes`` bytes; both are allocated when None.  No host synchronisation.  -> out."""
    require_gpu(vol, "vol")
    if vol.dim() != 3 or vol.dtype != _F32 or not vol.is_contiguous():
        raise ValueError("vol must be a contiguous float32 [nx,ny,nz] tensor")
    if int(n_iter) < 0:
        raise ValueError("n_iter must be >= 0")
    lo_f = float("-inf") if lo is None else float(lo)
    hi_f = float("inf") if hi is None else float(hi)
    if not lo_f <= hi_f:
        raise ValueError("the bounds must satisfy lo <= hi, got %r and %r" % (lo, hi))
    if out is None:
        out = torch.empty_like(vol)
    else:
        require_gpu(out, "out")
        if out.shape != vol.shape or out.dtype != _F32 or not out.is_contiguous() or out.device != vol.device:
            raise ValueError("out must be a contiguous float32 tensor of vol's shape on vol's device")
    nx, ny, nz = vol.shape
    nbytes = int(_lib.lib().r2_tv_prox_scratch_bytes(nx, ny, nz))
    if scratch is None:
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=vol.device)
    else:
        require_gpu(scratch, "scratch")
        if scratch.device != vol.device or not scratch.is_contiguous() or scratch.numel() * scratch.element_size() < nbytes:
            raise ValueError("scratch must be a contiguous buffer of at least %d bytes on vol's device" % nbytes)
    call("r2_tv_prox", vol.device, nx, ny, nz, vol, out, _scalar32(lam, vol.device), int(n_iter), lo_f, hi_f, scratch,
         scratch.numel() * scratch.element_size())
    return out


def tv_denoise(vol, lam, n_iter=50, lo=None, hi=None, device="cuda"):
    """``tv_prox`` for a host array (ROF denoising of a volume [nx,ny,nz]) -> numpy float32 array."""
    v = torch.as_tensor(np.ascontiguousarray(vol, dtype=np.float32)).to(device)
    return tv_prox(v, lam, n_iter, lo, hi, out=v).cpu().numpy()


def tv_value(x):
    """The isotropic, unsmoothed TV of ``tv_prox`` of a volume tensor: a float64 0-d tensor on its device."""
    x = x.to(_F64)
    sq = torch.zeros_like(x)
    sq[:-1] += (x[1:] - x[:-1]) ** 2
    sq[:, :-1] += (x[:, 1:] - x[:, :-1]) ** 2
    sq[:, :, :-1] += (x[:, :, 1:] - x[:, :, :-1]) ** 2
    return sq.sqrt().sum()


def operator_norm_bound(op):
    """max(A 1) max(A^T 1) = |A|_inf |A|_1 >= |A|_2^2: a guaranteed upper bound of the Lipschitz constant of
    x -> A^T (A x - b), because neither projector model has a negative entry.  A float32 0-d tensor on the device (no host
    read, nothing to tune)."""
    rows = op.A(torch.ones(op.nVoxel, dtype=_F32, device=op.device))
    cols = op.At(torch.ones((op.V, op.H, op.W), dtype=_F32, device=op.device))
    return rows.max() * cols.max()


def operator_norm_power(op, iters=20):
    """|A|_2^2 by ``iters`` steps of the power iteration on A^T A from the all-ones volume: the Rayleigh quotient
    |A v|^2 / |v|^2 of the last iterate, a LOWER estimate that converges from below (a step 1 / L with it may be too long;
    ``operator_norm_bound`` is the safe constant).  A float64 0-d tensor on the device."""
    if int(iters) < 1:
        raise ValueError("iters must be >= 1")
    v = torch.ones(op.nVoxel, dtype=_F32, device=op.device)
    est = torch.zeros((), dtype=_F64, device=op.device)
    for _ in range(int(iters)):
        v = v / torch.linalg.vector_norm(v, dtype=_F64).to(_F32)
        av = op.A(v)
        est = _sq(av)
        v = op.At(av)
    return est


def fista_tv(projs, angles, cfg, niter=50, lam=FISTA_LAM_REL, tviter=FISTA_TVITER, L=None, init=None, nonneg=True,
             computel2=False, accuracy=None, device="cuda", projection_type="interpolated", return_trace=False):
    """FISTA (Beck & Teboulle 2009) on  min_x 1/2 |A x - b|^2 + lambda TV(x), x >= 0 when ``nonneg``:  y_1 = x_0, t_1 = 1,

        x_k = tv_prox(y_k - (1 / L) A^T (A y_k - b), lambda / L, tviter, lo = 0 if nonneg),
        t_{k+1} = (1 + sqrt(1 + 4 t_k^2)) / 2,   y_{k+1} = x_k + ((t_k - 1) / t_{k+1}) (x_k - x_{k-1}).

    ``lam`` is relative: lambda = lam |A^T b|_inf, so that it does not depend on the units of b or the number of views.
    ``L``: None for ``operator_norm_bound`` (guaranteed >= |A|_2^2); a float or a 0-d device tensor is used as given.  lambda,
    L and lambda / L stay on the device and the dual of every ``tv_prox`` starts from zero: no iteration waits for the host
    unless ``computel2`` asks for the residual norms |A x_k - b|_2 (a host list).  -> x (GPU), or (x, l2) with computel2; with
    ``return_trace`` a dict comes last: ``lam`` (the absolute lambda), ``L``, and per iterate ``objective`` (index 0: at x_0),
    ``data`` = 1/2 |A x - b|^2 and ``tv``, float64 0-d device tensors."""
    op = Operator(angles, cfg, accuracy, device, projection_type)
    b = _projections(projs, op)
    if int(niter) < 0 or int(tviter) < 0:
        raise ValueError("niter and tviter must be >= 0")
    Lt = operator_norm_bound(op) if L is None else _scalar32(L, op.device)
    inv_L = (1.0 / Lt).to(_F32)
    lam_abs = (op.At(b).abs().max() * _scalar32(lam, op.device)).to(_F32)
    lam_L = lam_abs * inv_L
    x = _init(init, op)
    y = x.clone()
    z = torch.empty_like(x)
    x_new = torch.empty_like(x)
    res = torch.empty_like(b)
    g = torch.empty_like(x)
    scratch = torch.empty(int(_lib.lib().r2_tv_prox_scratch_bytes(*op.nVoxel)), dtype=torch.uint8, device=op.device)
    lo = 0.0 if nonneg else None
    trace = {"lam": lam_abs, "L": Lt, "objective": [], "data": [], "tv": []}

    def record(v):
        d, tv = 0.5 * _sq(op.A(v) - b), tv_value(v)
        trace["data"].append(d)
        trace["tv"].append(tv)
        trace["objective"].append(d + lam_abs.to(_F64) * tv)

    if return_trace:
        record(x)
    t = 1.0
    l2 = []
    for _ in range(int(niter)):
        op.A(y, out=res)
        res.sub_(b)
        op.At(res, out=g)
        torch.sub(y, g * inv_L, out=z)
        tv_prox(z, lam_L, tviter, lo, None, out=x_new, scratch=scratch)
        t_next = 0.5 * (1.0 + (1.0 + 4.0 * t * t) ** 0.5)
        torch.add(x_new, x_new - x, alpha=(t - 1.0) / t_next, out=y)
        x, x_new, t = x_new, x, t_next
        if computel2:
            l2.append(float(torch.linalg.vector_norm(op.A(x) - b, dtype=_F64)))
        if return_trace:
            record(x)
    out = (x, l2) if computel2 else (x,)
    if return_trace:
        out = out + (trace,)
    return out[0] if len(out) == 1 else out


# ---- the reference's entry points -------------------------------------------------------------------------------------------

def reconstruct(projs, angles, cfg, method, device="cuda", projection_type="interpolated"):
    """One of METHODS with the parameters ct_utils.py:60-175 passes -> x [nx,ny,nz] (GPU).  ``projection_type``: the model
    of the iterative methods' operator pair (FDK has none)."""
    pt = P.check_projection_type(projection_type)
    if method == "fdk":
        return F.fdk(projs, angles, cfg, device=device)
    if method == "sart":
        return sart(projs, angles, cfg, 20, 1.0, 0.999, device=device, projection_type=pt)
    if method == "ossart":
        return ossart(projs, angles, cfg, 20, 10, 1.0, 0.999, device=device, projection_type=pt)
    if method == "asd_pocs":
        return asd_pocs(projs, angles, cfg, 10, device=device, projection_type=pt)
    if method == "os_asd_pocs":
        return os_asd_pocs(projs, angles, cfg, 10, 10, device=device, projection_type=pt)
    if method == "cgls":
        return cgls(projs, angles, cfg, 60, device=device, projection_type=pt)
    if method == "fista_tv":
        return fista_tv(projs, angles, cfg, 50, device=device, projection_type=pt)
    raise NotImplementedError("Unsupported reconstruction method!")


def recon_volume(projs, angles, scanner_cfg, recon_method="fdk"):
    """ct_utils.py:17-27: ``"fdk"`` or ``"cgls"`` (60 iterations) -> numpy volume [nx,ny,nz]."""
    if recon_method not in ("fdk", "cgls"):
        raise ValueError("Unsupported reconstruction method")
    return reconstruct(projs, angles, scanner_cfg, recon_method).cpu().numpy()


def run_ct_recon_algs(projs, angles, cfg, ct_gt, save_path, method, projection_type="interpolated"):
    """ct_utils.py:60-215: reconstruct with ``method``, evaluate against ``ct_gt`` [nx,ny,nz] with ``metrics.metric_vol``, and
    write ``{save_path}/{method}/``: ct_gt.npy, ct_pred.npy, eval_3d.yml and slice_{method}/{i:05d}_gt.png / _pred.png
    (z slices).  -> (report, ct_pred, ct_gt), numpy volumes."""
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    import yaml
    from .metrics import metric_vol
    print("Run {}...".format(method))
    P.check_projection_type(projection_type)
    if method not in METHODS:
        raise NotImplementedError("Unsupported reconstruction method!")
    save_path = osp.join(save_path, method)
    slice_save_path = osp.join(save_path, "slice_{}".format(method))
    os.makedirs(slice_save_path, exist_ok=True)
    start = time.time()
    ct_pred = reconstruct(projs, angles, cfg, method, projection_type=projection_type).cpu().numpy()
    duration = time.time() - start
    ct_gt = np.asarray(ct_gt, dtype=np.float32)
    psnr_3d, _ = metric_vol(ct_gt, ct_pred, "psnr")
    ssim_3d, ssim_3d_axis = metric_vol(ct_gt, ct_pred, "ssim")
    np.save(osp.join(save_path, "ct_gt.npy"), ct_gt)
    np.save(osp.join(save_path, "ct_pred.npy"), ct_pred)
    for i in range(ct_gt.shape[2]):
        plt.imsave(osp.join(slice_save_path, "{0:05d}_gt.png".format(i)), ct_gt[:, :, i], cmap="gray", vmin=0.0, vmax=1.0)
        plt.imsave(osp.join(slice_save_path, "{0:05d}_pred.png".format(i)), ct_pred[:, :, i], cmap="gray", vmin=0.0,
                   vmax=1.0)
    report = {"method": method, "psnr_3d": float(psnr_3d), "ssim_3d": float(ssim_3d), "ssim_3d_x": float(ssim_3d_axis[0]),
              "ssim_3d_y": float(ssim_3d_axis[1]), "ssim_3d_z": float(ssim_3d_axis[2]), "duration (sec)": duration,
              "duration (min)": duration / 60}
    with open(osp.join(save_path, "eval_3d.yml"), "w") as f:
        yaml.dump(report, f, default_flow_style=False, sort_keys=False)
    print("[{}] psnr_3d: {}, ssim_3d: {}".format(method, psnr_3d, ssim_3d))
    return report, ct_pred, ct_gt


def _read_case(case_dir):
    """The case written by ``datagen.write_case``: raw config, projections and angles per split, the ground truth, and the
    reference reader's scene_scale (dataset_readers.py:62-76).  ``weights_train``: the recorded weights of the training
    projections, float32 [H, W] (shared by the views) or [V, H, W]; None for a case that records none."""
    with open(osp.join(case_dir, "meta_data.json"), "r", encoding="utf-8") as f:
        meta = json.load(f)
    cfg = meta["scanner"]
    out = {"cfg": cfg, "vol": np.load(osp.join(case_dir, meta["vol"])), "scale": 2.0 / max(cfg["sVoxel"])}
    for split in ("train", "test"):
        e = meta["proj_" + split]
        out[split] = (np.stack([np.load(osp.join(case_dir, x["file_path"])) for x in e]).astype(np.float32),
                      np.array([x["angle"] for x in e], dtype=np.float64))
    out["weights_train"] = None
    if "weights_train" in meta:
        w = np.load(osp.join(case_dir, meta["weights_train"])).astype(np.float32)
        if w.shape != out["train"][0].shape[1:] and w.shape != out["train"][0].shape:
            raise ValueError("weights_train is %s but the training projections are %s" % (w.shape, out["train"][0].shape))
        out["weights_train"] = w
    return out


def run_traditional_methods(source_path, model_path, methods=("fdk", "sart", "asd_pocs"), projection_type="interpolated"):
    """scripts/run_traditional_methods.py for a case in datagen's layout: every method's reconstruction and report, and its
    test-view projections ``{model_path}/{method}/projs/{i:05d}_render.npy/.png`` next to ``_gt.npy/.png``.  Like the
    reference (which reads them through Scene), the saved projections are in the normalised scene's units (times
    scene_scale).  ``projection_type``: the model of the reconstructions and of the test-view projections.  -> the dict
    written to ``{model_path}/eval_3d.yml``."""
    P.check_projection_type(projection_type)
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    import yaml
    case = _read_case(source_path)
    cfg, scale = case["cfg"], case["scale"]
    projs, angles = case["train"]
    test_projs, test_angles = case["test"]
    print("Run traditional algorithms on {}".format(osp.basename(osp.normpath(source_path))))
    out = {}
    for method in methods:
        out[method], ct_pred, _ = run_ct_recon_algs(projs, angles, cfg, case["vol"], model_path, method, projection_type)
        render = (P.project(ct_pred, test_angles, cfg, projection_type=projection_type) * scale).cpu().numpy()
        gt = test_projs * np.float32(scale)
        proj_save_path = osp.join(model_path, method, "projs")
        os.makedirs(proj_save_path, exist_ok=True)
        for i in range(render.shape[0]):
            np.save(osp.join(proj_save_path, "{0:05d}_render.npy".format(i)), render[i])
            np.save(osp.join(proj_save_path, "{0:05d}_gt.npy".format(i)), gt[i])
            plt.imsave(osp.join(proj_save_path, "{0:05d}_render.png".format(i)), render[i], cmap="gray")
            plt.imsave(osp.join(proj_save_path, "{0:05d}_gt.png".format(i)), gt[i], cmap="gray")
    with open(osp.join(model_path, "eval_3d.yml"), "w") as f:
        yaml.dump(out, f, default_flow_style=False, sort_keys=False)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description="Classical CT reconstructions of a case (run_traditional_methods.py)")
    ap.add_argument("-s", "--source_path", required=True, help="case directory as datagen writes it")
    ap.add_argument("-m", "--model_path", required=True, help="output directory")
    ap.add_argument("--methods", nargs="+", default=["fdk", "sart", "asd_pocs"], choices=METHODS)
    ap.add_argument("--projection_type", default="interpolated", choices=P.PROJECTION_TYPES,
                    help="projector model of the iterative methods and of the test-view projections")
    a = ap.parse_args(argv)
    run_traditional_methods(a.source_path, a.model_path, a.methods, a.projection_type)


if __name__ == "__main__":
    main()
