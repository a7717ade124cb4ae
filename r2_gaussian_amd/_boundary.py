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


def ptr_table(ts):
    """A ``void *[len(ts)]`` of the tensors' device pointers, NULL for None."""
    arr = (C.c_void_p * len(ts))()
    for i, t in enumerate(ts):
        arr[i] = None if t is None else t.data_ptr()
    return arr


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
