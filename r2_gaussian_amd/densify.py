"""Adaptive density control on the MI355X kernels (csrc/densify_ops.hip): the densification statistics of a
rendered view and ``densify_and_prune`` of r2_gaussian/gaussian/gaussian_model.py:320-556 -- clone, split, prune and the
Adam-state surgery -- without boolean-mask indexing (every ``x[mask]`` in the reference is a device synchronisation) and with
one host read per call (the new number of Gaussians).

Works on plain tensors; ``densify_and_prune_optimizer`` applies the result to a ``torch.optim.Adam`` whose four parameter groups
are named xyz / density / scaling / rotation like the reference's (gaussian_model.py:192-215).
"""
import ctypes as C

import torch

from . import _lib
from ._boundary import _F32, NAMES, call, require_gpu, rows_emit, rows_in


def densification_stats(radii, viewspace_grad, max_radii2D, grad_accum, denom):
    """In place (train.py:151-154, gaussian_model.py:552-556): for radii > 0: max_radii2D = max(., radii),
    grad_accum += ||viewspace_grad[:, :2]||, denom += 1.  One launch, no host synchronisation."""
    require_gpu(viewspace_grad, "viewspace_grad")
    P = radii.shape[0]
    assert viewspace_grad.shape == (P, 3) and viewspace_grad.is_contiguous() and radii.dtype == torch.int32
    for t in (max_radii2D, grad_accum, denom):
        assert t.numel() == P and t.is_contiguous() and t.dtype == _F32
    call("r2_densify_stats", viewspace_grad.device, P, radii.contiguous(), viewspace_grad, max_radii2D, grad_accum, denom)


def densification_stats_batch(radii, viewspace_grad, max_radii2D, grad_accum, denom, grad_scale=1.0):
    """`densification_stats` of the V views of a batched render in ONE launch: radii [V, P] int32 and viewspace_grad [V, P, 3] as
    GaussianRasterizerBatch leaves them.  Every view in order: for radii > 0: max_radii2D = max(., radii), grad_accum +=
    grad_scale * ||viewspace_grad[v, :, :2]||, denom += 1; with grad_scale 1 bit-identical to V single-view calls.
    grad_scale = V undoes the 1 / V a mean-over-views loss leaves in the gradients (exact for V a power of two)."""
    require_gpu(viewspace_grad, "viewspace_grad")
    if radii.dim() != 2 or radii.shape[0] < 1:
        raise ValueError("radii must be [V, P] with V >= 1, got %s" % (tuple(radii.shape),))
    V, P = radii.shape
    assert viewspace_grad.shape == (V, P, 3) and viewspace_grad.is_contiguous() and viewspace_grad.dtype == _F32
    assert radii.dtype == torch.int32
    for t in (max_radii2D, grad_accum, denom):
        assert t.numel() == P and t.is_contiguous() and t.dtype == _F32
    call("r2_densify_stats_batch", viewspace_grad.device, P, V, radii.contiguous(), viewspace_grad, float(grad_scale), max_radii2D,
         grad_accum, denom)


def densify_and_prune(params, moments, max_radii2D, grad_accum, denom, normals, grad_threshold, scale_threshold, density_min,
                      bbox, scale_bound=None, do_densify=True, max_screen_size=None, max_scale=None):
    """params: dict name -> raw parameter tensor ([P,3], [P,1], [P,3], [P,4]); moments: dict name -> (exp_avg, exp_avg_sq) or
    None; normals: [2,P,3] N(0,1).  -> (new_params, new_moments, new_max_radii2D, new_grad_accum, new_denom, counts) with
    rows ordered like the reference's result; counts = surviving (originals, clones, first children, second children).
    max_screen_size / max_scale: the reference's optional prune thresholds (gaussian_model.py:540-545; None / 0 = off):
    rows whose max_radii2D exceeds the first or whose largest activated scale exceeds the second are pruned -- children of a
    split inherit the parent's max_radii2D and get its scale / 1.6.  Raises ValueError when nothing survives (train.py:169-172)."""
    xyz = params["xyz"]
    require_gpu(xyz, "xyz")
    dev, P = xyz.device, xyz.shape[0]
    L = _lib.lib()
    if moments is not None and any(moments.get(n) is None for n in NAMES):
        moments = None
    rows = rows_in(params, moments, (max_radii2D, grad_accum, denom), P, dev)
    ps, (mr, ga, dn) = rows[0], rows[3]
    nrm = normals.to(device=dev, dtype=_F32).contiguous()
    assert nrm.shape == (2, P, 3)
    lo, hi = (float(scale_bound[0]), float(scale_bound[1])) if scale_bound is not None else (1.0, 0.0)
    box = (C.c_float * 6)(*[float(v) for v in torch.as_tensor(bbox).reshape(-1).tolist()])
    scratch = torch.empty(L.r2_densify_scratch_bytes(P), dtype=torch.uint8, device=dev)
    counts = (C.c_uint * 4)()
    common = (float(grad_threshold), float(scale_threshold), float(density_min), box, lo, hi, int(bool(do_densify)),
              float(max_screen_size or 0.0), float(max_scale or 0.0))
    call("r2_densify_classify", dev, P, *ps, mr, ga, dn, nrm, *common, scratch, counts)
    cnt = tuple(int(c) for c in counts)
    Pn = sum(cnt)
    if Pn == 0:
        raise ValueError("No Gaussian left. Change adaptive control hyperparameters!")   # train.py:169-172
    new_params, new_moments, (mro, gao, dno) = rows_emit(Pn, dev, rows, lambda tin, tout, so: call(
        "r2_densify_emit", dev, P, *tin, mr, ga, dn, nrm, *common, scratch, *tout, *so))
    return new_params, new_moments, mro, gao, dno, cnt


def densify_and_prune_optimizer(optimizer, max_radii2D, grad_accum, denom, normals, grad_threshold, scale_threshold,
                                density_min, bbox, scale_bound=None, do_densify=True, max_screen_size=None, max_scale=None):
    """The same on a ``torch.optim.Adam`` with parameter groups named xyz / density / scaling / rotation (one tensor each):
    parameters and ``exp_avg`` / ``exp_avg_sq`` are replaced like cat_tensors_to_optimizer / _prune_optimizer do
    (gaussian_model.py:335-403).  -> (dict name -> new parameter, new max_radii2D, new grad_accum [P,1], new denom [P,1])."""
    groups = {g["name"]: g for g in optimizer.param_groups}
    params = {n: groups[n]["params"][0] for n in NAMES}
    states = {n: optimizer.state.get(params[n]) for n in NAMES}
    moments = {n: (states[n]["exp_avg"], states[n]["exp_avg_sq"]) for n in NAMES} if all(
        s is not None and "exp_avg" in s for s in states.values()) else None
    new_p, new_m, mr, ga, dn, _cnt = densify_and_prune(params, moments, max_radii2D, grad_accum, denom, normals, grad_threshold,
                                                       scale_threshold, density_min, bbox, scale_bound, do_densify,
                                                       max_screen_size, max_scale)
    out = {}
    for n in NAMES:
        old = params[n]
        st = optimizer.state.pop(old, None)
        p = torch.nn.Parameter(new_p[n].requires_grad_(True))
        groups[n]["params"][0] = p
        if st is not None:
            if new_m is not None:
                st["exp_avg"], st["exp_avg_sq"] = new_m[n]
            optimizer.state[p] = st
        out[n] = p
    return out, mr, ga.reshape(-1, 1), dn.reshape(-1, 1)
