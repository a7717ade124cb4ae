"""How Python talks to libr2hip.so, in one place: every stream-taking entry of the C ABI (include/r2hip.h) is reached through
``call``, which owns the device switch, the tensor -> device pointer conversion, the current HIP stream and the return-code
convention, so that a call site names its symbol once and spells out nothing but its arguments.  The small conversions the
sites share (``f32c``, ``cloud``, ``ptr_table``) live next to it.  ``_lib`` stays free of torch; this module is its torch half.
"""
import ctypes as C

import torch

from . import _lib

_F32 = torch.float32
_Tensor = torch.Tensor


def require_gpu(t, name):
    if not t.is_cuda:
        raise _lib.R2HipError("%s must be a GPU tensor: the MI355X kernels have no CPU fallback" % name)


class on_device:
    """``with torch.cuda.device(dev)`` only when dev is not already current (the context manager costs ~10 us)."""

    __slots__ = ("ctx",)

    def __init__(self, dev):
        self.ctx = None if torch.cuda.current_device() == (dev.index or 0) else torch.cuda.device(dev)

    def __enter__(self):
        if self.ctx is not None:
            self.ctx.__enter__()

    def __exit__(self, *a):
        if self.ctx is not None:
            self.ctx.__exit__(*a)


def stream(device):
    return torch.cuda.current_stream(device).cuda_stream


def f32c(t):
    return t if t.dtype == _F32 and t.is_contiguous() else t.to(_F32).contiguous()


def cloud(xyz, density, scaling, rotation):
    """The four parameter tensors as the kernels read them: detached, contiguous, float32 (the tensors themselves where they
    already are), in the caller's shapes."""
    return f32c(xyz.detach()), f32c(density.detach()), f32c(scaling.detach()), f32c(rotation.detach())


NAMES = ("xyz", "density", "scaling", "rotation")                     # the cloud's parameter groups, in the ABI's order ...
WIDTHS = {"xyz": 3, "density": 1, "scaling": 3, "rotation": 4}        # ... and the floats of a row of each


def cloud_checked(ts, P, dev, names=NAMES, what="", gpu=True):
    """The tensors of the groups ``names`` as the kernels read them: [P, width] on ``dev`` (a density may be [P]) -> detached
    contiguous float32 [P, width]; ValueError for another shape or device, with ``gpu`` R2HipError for a CPU tensor."""
    out = []
    for name, t in zip(names, ts):
        if gpu:
            require_gpu(t, name)
        if name == "density" and t.ndim == 1:
            t = t[:, None]
        if tuple(t.shape) != (P, WIDTHS[name]) or t.device != dev:
            raise ValueError("%s%s must be [%d, %d] on %s, got %s on %s" % (what, name, P, WIDTHS[name], dev, tuple(t.shape), t.device))
        out.append(f32c(t.detach()))
    return out


def ptr_table(ts):
    """A ``void *[len(ts)]`` of the tensors' device pointers, NULL for None."""
    arr = (C.c_void_p * len(ts))()
    for i, t in enumerate(ts):
        arr[i] = None if t is None else t.data_ptr()
    return arr


def rows_in(params, moments, stats, P, dev):
    """The rows of a cloud as an emit-type entry (r2_densify_emit, r2_relocate_emit) reads them.  params: dict name -> raw
    parameter [P, width]; moments: dict name -> (exp_avg, exp_avg_sq), or None; stats: (max_radii2D, grad_accum, denom) of P
    elements each, or None.  -> (ps, ms, vs, st): contiguous float32, ms / vs / st None where not given; ValueError for a shape
    or a device that does not fit."""
    ps = cloud_checked([params[n] for n in NAMES], P, dev, gpu=False)
    ms = vs = st = None
    if moments is not None:
        ms, vs = (cloud_checked([moments[n][k] for n in NAMES], P, dev, what="a moment of ", gpu=False) for k in (0, 1))
    if stats is not None:
        st = [f32c(t.detach()).reshape(-1) for t in stats]
        if len(st) != 3 or any(t.numel() != P or t.device != dev for t in st):
            raise ValueError("stats must be (max_radii2D, grad_accum, denom) with %d elements each on %s" % (P, dev))
    return ps, ms, vs, st


def rows_emit(Pn, dev, rows, emit):
    """Allocates the Pn-row outputs of ``rows`` (rows_in's tuple; moments and statistics only where given) and runs
    ``emit(tables_in, tables_out, stats_out)``: the pointer tables of (parameters, exp_avg, exp_avg_sq), None for an absent
    one, and the three output statistics or Nones.  -> (new_params, new_moments or None, new_stats or None)."""
    ps, ms, vs, st = rows
    po, mo, vo = ([torch.empty((Pn, w), dtype=_F32, device=dev) for w in WIDTHS.values()] if g is not None else None
                  for g in (ps, ms, vs))
    so = [torch.empty((Pn,), dtype=_F32, device=dev) for _ in range(3)] if st is not None else None
    table = lambda g: None if g is None else ptr_table(g)   # noqa: E731
    emit([table(g) for g in (ps, ms, vs)], [table(g) for g in (po, mo, vo)], so if st is not None else [None] * 3)
    new_moments = {n: (m, v) for n, m, v in zip(NAMES, mo, vo)} if ms is not None else None
    return dict(zip(NAMES, po)), new_moments, (tuple(so) if st is not None else None)


def workspace(nbytes, dev, at_least=0):
    """The library does not allocate: a byte buffer of the size one of its ``*_workspace_bytes`` sizers asks for, from torch's
    allocator.  ``at_least=1`` where the entry wants a real pointer even for zero bytes."""
    return torch.empty((max(int(nbytes), at_least),), dtype=torch.uint8, device=dev)


def call(name, dev, *args):
    """``name(*args, stream)`` of libr2hip.so on ``dev`` and its current stream: tensors among ``args`` go down as their device
    pointers, None as NULL, everything else as it is.  -> the entry's non-negative result; R2HipError, with the library's
    text, for a negative one.  Stateless, so safe from several threads at once (multistream.StreamPool)."""
    fn = getattr(_lib.lib(), name)
    with on_device(dev):
        rc = fn(*[a.data_ptr() if isinstance(a, _Tensor) else a for a in args], stream(dev))
    return _lib.check(rc, name)
