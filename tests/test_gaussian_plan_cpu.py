"""CPU: the C ABI of the projection plans (include/r2hip.h, "projection plans"; csrc/gaussian_plan.hip and the *_planned
entries of the five pixel-major operators): the symbols, the workspace sizer and the argument checks, which precede every HIP
call and so run without a GPU."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

BUILD = ("r2_project_gaussians_plan_workspace_bytes", "r2_project_gaussians_plan_count", "r2_project_gaussians_plan_fill")
PLANNED = ("r2_project_gaussians_planned", "r2_project_gaussians_rays_backward_planned", "r2_project_gaussians_variance_planned",
           "r2_project_gaussians_jvp_planned", "r2_project_gaussians_ray_jacobian_planned")


def test_symbols_are_declared_and_exported():
    from r2_gaussian_amd import _lib
    with open(os.path.join(ROOT, "include", "r2hip.h")) as f:
        header = f.read()
    L = _lib.lib()
    for name in BUILD + PLANNED:
        assert re.search(r"R2_API\s+\w+\s+%s\(" % name, header), name
        assert name in _lib.exported_symbols()
        assert getattr(L, name) is not None
    assert re.search(r"R2_ABI_VERSION\s+3\b", header) and L.r2_abi_version() == 3


def test_workspace_bytes_is_monotone_and_zero_without_gaussians():
    from r2_gaussian_amd import _lib
    size = _lib.lib().r2_project_gaussians_plan_workspace_bytes
    assert size(3, 70, 50, 0) == 0 and size(0, 70, 50, 10) == 0
    last = 0
    for V in (1, 2, 3, 8):
        assert size(V, 70, 50, 300) > last
        last = size(V, 70, 50, 300)
    last = 0
    for P in (1, 2, 255, 256, 257, 50000):
        assert size(2, 70, 50, P) > last
        last = size(2, 70, 50, P)


def _buffers():
    """Host memory that stands for every pointer: the checks under test return before anything is dereferenced."""
    f = (C.c_float * 64)()
    return C.addressof(f), f


# name -> (builder of the argument list from V, rays, out; the position the entry keeps its stream in is the last)
def _calls(p):
    cloud = lambda: (p, p, p, 1.0, p)
    return {
        "r2_project_gaussians_plan_count": lambda V, rays, out: (V, 8, 8, rays, 1, 1, *cloud(), out, p, 1 << 20, None),
        "r2_project_gaussians_plan_fill": lambda V, rays, out: (V, 8, 8, rays, 1, 1, *cloud(), p, out, 4, p, 1 << 20, None),
        "r2_project_gaussians_planned": lambda V, rays, out: (V, 8, 8, rays, 1, 1, *cloud(), out, p, p, 4, None),
        "r2_project_gaussians_rays_backward_planned": lambda V, rays, out: (V, 8, 8, rays, 1, 1, *cloud(), p, out, p, 1 << 20, p, p,
                                                                            4, None),
        "r2_project_gaussians_variance_planned": lambda V, rays, out: (V, 8, 8, rays, 1, 1, *cloud(), p, p, p, p, out, p, p, 4, None),
        "r2_project_gaussians_jvp_planned": lambda V, rays, out: (V, 8, 8, rays, 1, 1, *cloud(), p, p, p, p, out, p, p, 4, None),
        "r2_project_gaussians_ray_jacobian_planned": lambda V, rays, out: (V, 8, 8, rays, 1, 1, *cloud(), out, p, p, 4, None),
    }


@pytest.mark.parametrize("name", BUILD[1:] + PLANNED)
def test_invalid_arguments_are_refused_before_any_hip_call(name):
    """V = 0, a NULL rays and a NULL out (the offsets of the count, the ids of the fill with a capacity of 4) each give
    R2_ERR_INVALID and a message that names the entry."""
    from r2_gaussian_amd import _lib
    L = _lib.lib()
    p, keep = _buffers()
    call = _calls(p)[name]
    for what, args in (("V = 0", call(0, p, p)), ("NULL rays", call(1, None, p)), ("NULL out", call(1, p, None))):
        rc = getattr(L, name)(*args)
        assert rc == _lib.R2_ERR_INVALID, (name, what)
        assert name + ":" in L.r2_last_error().decode(), (name, what, L.r2_last_error())
    del keep


@pytest.mark.parametrize("name", PLANNED + BUILD[2:])
def test_missing_lists_are_refused_before_any_hip_call(name):
    """A NULL offsets pointer, a NULL ids pointer with a capacity above 0 and a negative capacity, with P = 1."""
    from r2_gaussian_amd import _lib
    L = _lib.lib()
    p, keep = _buffers()
    args = list(_calls(p)[name](1, p, p))
    if name.endswith("plan_fill"):
        off, ids, cap = 11, 12, 13
    else:
        off, ids, cap = len(args) - 4, len(args) - 3, len(args) - 2
    assert args[cap] == 4
    for what, pos, value in (("NULL offsets", off, None), ("NULL ids", ids, None), ("negative capacity", cap, -1)):
        bad = list(args)
        bad[pos] = value
        rc = getattr(L, name)(*bad)
        assert rc == _lib.R2_ERR_INVALID and name + ":" in L.r2_last_error().decode(), (name, what)
    del keep


@pytest.mark.parametrize("name", BUILD[1:])
def test_a_small_workspace_names_the_sizer(name):
    from r2_gaussian_amd import _lib
    L = _lib.lib()
    p, keep = _buffers()
    args = list(_calls(p)[name](1, p, p))
    need = L.r2_project_gaussians_plan_workspace_bytes(1, 8, 8, 1)
    assert need > 0
    for ws, size in ((p, need - 1), (None, 1 << 20)):
        bad = list(args)
        bad[-3], bad[-2] = ws, size
        rc = getattr(L, name)(*bad)
        msg = L.r2_last_error().decode()
        assert rc == _lib.R2_ERR_INVALID and name + ":" in msg and "r2_project_gaussians_plan_workspace_bytes" in msg, (name, msg)
    del keep
