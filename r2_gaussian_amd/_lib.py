"""ctypes binding of libr2hip.so (the C ABI declared in include/r2hip.h).

The product path has NO fallback: if the HIP library is missing or fails to load, importing the ops
raises.  Build it with ``python -m r2_gaussian_amd.build`` (or ``__graft_entry__.build()``).
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# R2HIP_LIB selects an experiment build (profiling ablations); the default is the product library
LIB_PATH = os.environ.get("R2HIP_LIB") or os.path.join(_HERE, "libr2hip.so")

ALLOC_FN = C.CFUNCTYPE(C.c_void_p, C.c_size_t, C.c_void_p)

R2_ABI_VERSION = 3
R2_ERR_INVALID = -10001
R2_ERR_ALLOC = -10002
R2_METRIC_SSIM = 1
R2_METRIC_NORMALIZE = 2
R2_LOSS_BATCH_CHUNK = 16
R2_KNN_GRAPH_MAX_K = 16
R2_GRAPH_KIND_L1, R2_GRAPH_KIND_L2, R2_GRAPH_KIND_HUBER = 0, 1, 2
R2_GRAPH_LOSS_CHAIN = 17   # longest chain of float roundings in r2_graph_loss's reduction (include/r2hip.h)
R2_GRAPH_LOSS_HUB = 64     # incoming lists longer than this are summed by a whole wave in r2_graph_loss_backward
R2_MERGE_HUB = 64          # ... and walked by a whole wave in r2_graph_match / r2_merge_count
R2_MERGE_JACOBI_SWEEPS = 8
R2_RELOCATE_SCAN_TILE = 4096   # elements per workgroup of r2_relocate_plan's 64-bit scan
R2_SPLINE_PAD = 12             # edge padding of r2_spline_prefilter's coefficient block, per side
R2_SPLINE_HORIZON = 16         # terms of its start sum

_f, _i, _p, _fp = C.c_float, C.c_int, C.c_void_p, C.c_void_p

_SIGNATURES = {
    "r2_abi_version": (C.c_int, []),
    "r2_last_error": (C.c_char_p, []),
    "r2_raster_forward": (C.c_int, [ALLOC_FN, _p, ALLOC_FN, _p, ALLOC_FN, _p, _i, _i, _i, _fp, _fp, _fp, _f, _fp, _fp,
                                    _fp, _fp, _fp, _f, _f, _i, _i, _fp, _p, _i, _p]),
    "r2_raster_backward": (C.c_int, [_i, _i, _i, _i, _fp, _fp, _f, _fp, _fp, _fp, _fp, _fp, _f, _f, _p, _p, _p, _p,
                                     _fp, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _i, _i, _p]),
    "r2_mark_visible": (C.c_int, [_i, _fp, _fp, _fp, _p, _p]),
    "r2_raster_forward_batch": (C.c_int, [ALLOC_FN, _p, ALLOC_FN, _p, ALLOC_FN, _p, _i, _i, _i, _i, _fp, _fp, _fp, _f, _fp,
                                          _fp, _fp, _fp, _f, _f, _i, _fp, _p, _i, _p]),
    "r2_raster_backward_batch": (C.c_int, [_i, _i, _i, _i, _i, _fp, _fp, _f, _fp, _fp, _fp, _fp, _f, _f, _p, _p, _p, _p,
                                           _fp, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _i, _i, _p]),
    "r2_voxel_forward": (C.c_int, [ALLOC_FN, _p, ALLOC_FN, _p, ALLOC_FN, _p, _i, _i, _i, _i, _f, _f, _f, _f, _f, _f,
                                   _fp, _fp, _fp, _f, _fp, _fp, _i, _fp, _p, _p, _p, _i, _p]),
    "r2_voxel_backward": (C.c_int, [_i, _i, _i, _i, _i, _f, _f, _f, _f, _f, _f, _fp, _fp, _f, _fp, _fp, _p, _p, _p,
                                    _p, _p, _p, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _i, _p]),
    "r2_voxel_forward_slab": (C.c_int, [ALLOC_FN, _p, ALLOC_FN, _p, ALLOC_FN, _p, _i, _i, _i, _i, _f, _f, _f, _f, _f, _f, _i, _i,
                                        _fp, _fp, _fp, _f, _fp, _fp, _i, _fp, _p, _p, _p, _i, _p]),
    "r2_voxel_backward_slab": (C.c_int, [_i, _i, _i, _i, _i, _f, _f, _f, _f, _f, _f, _i, _i, _fp, _fp, _f, _fp, _fp, _p, _p, _p,
                                         _p, _p, _p, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _i, _p]),
    "r2_knn_dist2": (C.c_int, [_i, _fp, _fp, _p]),
    "r2_knn_workspace_bytes": (C.c_size_t, [_i]),
    "r2_knn_dist2_ws": (C.c_int, [_i, _fp, _fp, _p, C.c_size_t, _p]),
    "r2_knn_graph_workspace_bytes": (C.c_size_t, [_i, _i]),
    "r2_knn_graph": (C.c_int, [_i, _fp, _i, _p, _fp, _p, C.c_size_t, _p]),
    "r2_graph_transpose_workspace_bytes": (C.c_size_t, [_i, _i]),
    "r2_graph_transpose": (C.c_int, [_i, _i, _p, _p, _p, _p, C.c_size_t, _p]),
    "r2_graph_loss_scratch_floats": (C.c_size_t, [_i, _i]),
    "r2_graph_loss": (C.c_int, [_i, _i, _fp, _p, _fp, _i, _f, _f, _fp, _fp, _p]),
    "r2_graph_loss_backward": (C.c_int, [_i, _i, _fp, _p, _fp, _p, _p, _i, _f, _f, _fp, _fp, _p]),
    "r2_merge_cost": (C.c_int, [_i, _i, _p, _fp, _fp, _fp, _fp, _f, _fp, _p]),
    "r2_graph_match_workspace_bytes": (C.c_size_t, [_i]),
    "r2_graph_match": (C.c_int, [_i, _i, _p, _p, _p, _fp, _f, _i, _p, _p, C.c_size_t, _p]),
    "r2_merge_scratch_bytes": (C.c_size_t, [_i]),
    "r2_merge_count": (C.c_int, [_i, _i, _p, _p, _p, _fp, _f, _p, _fp, _fp, _p, _p, _p]),
    "r2_merge_emit": (C.c_int, [_i, _fp, _fp, _fp, _fp, _p, _i, _fp, _fp, _fp, _fp, _p, _p]),
    "r2_gaussian_noise": (C.c_int, [_i, _fp, _fp, _fp, _fp, C.c_double, _f, _f, C.c_ulonglong, C.c_ulonglong, _p]),
    "r2_relocate_workspace_bytes": (C.c_size_t, [_i, _i]),
    "r2_relocate_plan": (C.c_int, [_i, _i, _p, _fp, _fp, _f, C.c_ulonglong, C.c_ulonglong, _p, _p, _p, C.c_size_t, _p, _p]),
    "r2_relocate_emit": (C.c_int, [_i, _i, _p, _p, _p, _fp, _fp, _fp, _fp, _fp, _fp, _f, C.c_ulonglong, C.c_ulonglong, _p, _p,
                                   _p, C.c_size_t, _p, _p, _p, _fp, _fp, _fp, _p]),
    "r2_tile_first_stats": (None, [C.POINTER(C.c_longlong), _i]),
    "r2_defer_count_control": (None, [_i]),
    "r2_defer_count_resolve": (C.c_int, [_i, C.POINTER(C.c_int), _p]),
    "r2_defer_count_stats": (None, [C.POINTER(C.c_longlong), _i]),
    "r2_voxel_sticks_control": (None, [_i]),
    "r2_voxel_sticks_limits": (None, [C.c_longlong, C.c_longlong]),
    "r2_voxel_sticks_stats": (None, [C.POINTER(C.c_longlong), _i]),
    "r2_thread_release": (None, []),
    "r2_path_stat_count": (C.c_int, []),
    "r2_path_stat_name": (C.c_char_p, [_i]),
    "r2_path_stats": (C.c_int, [C.POINTER(C.c_longlong), _i, _i]),
    "r2_densify_stats": (C.c_int, [_i, _p, _fp, _fp, _fp, _fp, _p]),
    "r2_densify_stats_batch": (C.c_int, [_i, _i, _p, _fp, _f, _fp, _fp, _fp, _p]),
    "r2_densify_scratch_bytes": (C.c_size_t, [_i]),
    "r2_densify_classify": (C.c_int, [_i, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _f, _f, _f, _p, _f, _f, _i, _f, _f, _p, _p, _p]),
    "r2_densify_emit": (C.c_int, [_i, _p, _p, _p, _fp, _fp, _fp, _fp, _f, _f, _f, _p, _f, _f, _i, _f, _f, _p, _p, _p, _p, _fp,
                                  _fp, _fp, _p]),
    "r2_loss_l1_ssim_scratch_floats": (C.c_size_t, [_i, _i]),
    "r2_loss_l1_ssim": (C.c_int, [_i, _i, _fp, _fp, _f, _f, _fp, _fp, _fp, _p]),
    "r2_loss_l1_ssim_batch_scratch_floats": (C.c_size_t, [_i, _i, _i]),
    "r2_loss_l1_ssim_batch": (C.c_int, [_i, _i, _i, _fp, _p, _f, _f, _fp, _fp, _fp, _p]),
    "r2_loss_l1_ssim_weighted_scratch_floats": (C.c_size_t, [_i, _i]),
    "r2_loss_l1_ssim_weighted": (C.c_int, [_i, _i, _fp, _fp, _fp, _f, _f, _fp, _fp, _fp, _p]),
    "r2_loss_l1_ssim_weighted_batch_scratch_floats": (C.c_size_t, [_i, _i, _i]),
    "r2_loss_l1_ssim_weighted_batch": (C.c_int, [_i, _i, _i, _fp, _p, _p, _f, _f, _fp, _fp, _fp, _p]),
    "r2_loss_tv3d_scratch_floats": (C.c_size_t, [_i, _i, _i]),
    "r2_loss_tv3d": (C.c_int, [_i, _i, _i, _fp, _f, _fp, _fp, _fp, _p]),
    "r2_metric_slices_scratch_floats": (C.c_size_t, [_i, _i, _i, _i]),
    "r2_metric_slices": (C.c_int, [_i, _i, _i, _i, _fp, _fp, _i, _fp, _fp, _p]),
    "r2_fdk_filter": (C.c_int, [_i, _i, _i, _fp, _fp, _f, _i, _f, _f, _f, _fp, _p]),
    "r2_fdk_backproject": (C.c_int, [_i, _i, _i, _fp, _fp, _i, _f, _i, _i, _i, _f, _f, _f, _f, _f, _f, _fp, _p]),
    "r2_project_volume": (C.c_int, [_i, _i, _i, _fp, _i, _i, _i, _i, _f, _f, _f, _f, _fp, _fp, _p]),
    "r2_backproject_volume": (C.c_int, [_i, _i, _i, _fp, _i, _i, _i, _i, _f, _f, _f, _f, _fp, _fp, _p]),
    "r2_project_volume_siddon": (C.c_int, [_i, _i, _i, _fp, _i, _i, _i, _i, _f, _f, _f, _fp, _fp, _p]),
    "r2_backproject_volume_siddon": (C.c_int, [_i, _i, _i, _fp, _i, _i, _i, _i, _f, _f, _f, _fp, _fp, _p]),
    "r2_project_gaussians": (C.c_int, [_i, _i, _i, _fp, _i, _i, _fp, _fp, _fp, _f, _fp, _fp, _p]),
    "r2_project_gaussians_backward": (C.c_int, [_i, _i, _i, _fp, _i, _i, _fp, _fp, _fp, _f, _fp, _fp, _fp, _fp, _fp, _fp, _p]),
    "r2_project_gaussians_rays_backward_workspace_bytes": (C.c_size_t, [_i, _i, _i]),
    "r2_project_gaussians_rays_backward": (C.c_int, [_i, _i, _i, _fp, _i, _i, _fp, _fp, _fp, _f, _fp, _fp, _fp, _p, C.c_size_t, _p]),
    "r2_query_gaussians": (C.c_int, [_i, _fp, _i, _fp, _fp, _fp, _f, _fp, _fp, _p]),
    "r2_query_gaussians_workspace_bytes": (C.c_size_t, [_i]),
    "r2_query_gaussians_backward": (C.c_int, [_i, _fp, _i, _fp, _fp, _fp, _f, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _p, C.c_size_t, _p]),
    "r2_integrate_gaussians": (C.c_int, [_i, _fp, _i, _i, _fp, _fp, _fp, _f, _fp, _fp, _p, C.c_size_t, _p]),
    "r2_integrate_gaussians_workspace_bytes": (C.c_size_t, [_i, _i]),
    "r2_integrate_gaussians_backward": (C.c_int, [_i, _fp, _i, _i, _fp, _fp, _fp, _f, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _p,
                                                  C.c_size_t, _p]),
    "r2_integrate_gaussians_leaves": (C.c_int, [_i, _fp, _i, _i, _fp, _fp, _fp, _f, _fp, _fp, _p, C.c_size_t, _p]),
    "r2_integrate_gaussians_leaves_workspace_bytes": (C.c_size_t, [_i, _i]),
    "r2_integrate_gaussians_leaves_backward": (C.c_int, [_i, _fp, _i, _i, _fp, _fp, _fp, _f, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _p,
                                                         C.c_size_t, _p]),
    "r2_project_gaussians_fisher": (C.c_int, [_i, _i, _i, _fp, _i, _i, _fp, _fp, _fp, _f, _fp, _fp, _fp, _fp, _fp, _fp, _p]),
    "r2_query_gaussians_variance": (C.c_int, [_i, _fp, _i, _fp, _fp, _fp, _f, _fp, _fp, _fp, _fp, _fp, _fp, _p]),
    "r2_project_gaussians_variance": (C.c_int, [_i, _i, _i, _fp, _i, _i, _fp, _fp, _fp, _f, _fp, _fp, _fp, _fp, _fp, _fp, _p]),
    "r2_project_gaussians_jvp": (C.c_int, [_i, _i, _i, _fp, _i, _i, _fp, _fp, _fp, _f, _fp, _fp, _fp, _fp, _fp, _fp, _p]),
    "r2_project_gaussians_ray_jacobian": (C.c_int, [_i, _i, _i, _fp, _i, _i, _fp, _fp, _fp, _f, _fp, _fp, _p]),
    "r2_project_gaussians_plan_workspace_bytes": (C.c_size_t, [_i, _i, _i, _i]),
    "r2_project_gaussians_plan_count": (C.c_int, [_i, _i, _i, _fp, _i, _i, _fp, _fp, _fp, _f, _fp, _p, _p, C.c_size_t, _p]),
    "r2_project_gaussians_plan_fill": (C.c_int, [_i, _i, _i, _fp, _i, _i, _fp, _fp, _fp, _f, _fp, _p, _p, C.c_longlong, _p,
                                                 C.c_size_t, _p]),
    "r2_project_gaussians_planned": (C.c_int, [_i, _i, _i, _fp, _i, _i, _fp, _fp, _fp, _f, _fp, _fp, _p, _p, C.c_longlong, _p]),
    "r2_project_gaussians_rays_backward_planned": (C.c_int, [_i, _i, _i, _fp, _i, _i, _fp, _fp, _fp, _f, _fp, _fp, _fp, _p,
                                                             C.c_size_t, _p, _p, C.c_longlong, _p]),
    "r2_project_gaussians_variance_planned": (C.c_int, [_i, _i, _i, _fp, _i, _i, _fp, _fp, _fp, _f, _fp, _fp, _fp, _fp, _fp, _fp,
                                                        _p, _p, C.c_longlong, _p]),
    "r2_project_gaussians_jvp_planned": (C.c_int, [_i, _i, _i, _fp, _i, _i, _fp, _fp, _fp, _f, _fp, _fp, _fp, _fp, _fp, _fp,
                                                   _p, _p, C.c_longlong, _p]),
    "r2_project_gaussians_ray_jacobian_planned": (C.c_int, [_i, _i, _i, _fp, _i, _i, _fp, _fp, _fp, _f, _fp, _fp, _p, _p,
                                                            C.c_longlong, _p]),
    "r2_tv_descent_scratch_bytes": (C.c_size_t, [_i, _i, _i]),
    "r2_tv_descent": (C.c_int, [_i, _i, _i, _fp, _fp, _i, _p, C.c_size_t, _p]),
    "r2_tv_prox_scratch_bytes": (C.c_size_t, [_i, _i, _i]),
    "r2_tv_prox": (C.c_int, [_i, _i, _i, _fp, _fp, _fp, _i, _f, _f, _p, C.c_size_t, _p]),
    "r2_isosurface_workspace_bytes": (C.c_size_t, [_i, _i, _i]),
    "r2_isosurface_count": (C.c_int, [_i, _i, _i, _fp, _f, _p, C.c_size_t, _p, _p]),
    "r2_isosurface_fill": (C.c_int, [_i, _i, _i, _fp, _f, _f, _f, _f, _f, _f, _f, _p, C.c_size_t, C.c_longlong, C.c_longlong,
                                     _fp, _fp, _p, _p]),
    "r2_spline_prefilter": (C.c_int, [_i, _i, _i, _fp, _fp, _p]),
    "r2_spline_prefilter_pass": (C.c_int, [_i, _i, _i, _fp, _fp, _i, _p]),
    "r2_spline_zoom_workspace_bytes": (C.c_size_t, [_i, _i, _i]),
    "r2_spline_zoom": (C.c_int, [_i, _i, _i, _fp, _i, _i, _i, _fp, _p, C.c_size_t, _p]),
    "r2_spline_sample": (C.c_int, [_i, _i, _i, _fp, _i, _fp, _fp, _p]),
    "r2_proj_resize_workspace_bytes": (C.c_size_t, [_i, _i]),
    "r2_proj_resize": (C.c_int, [_i, _i, _i, _fp, _i, _i, _f, _i, _i, _i, _i, _i, _i, _i, _fp, _p, C.c_size_t, _p]),
    "r2_proj_median": (C.c_int, [_i, _i, _i, _fp, _i, _i, _f, _fp, _p, _p]),
    "r2_proj_destripe_max_views": (C.c_int, []),
    "r2_proj_destripe_workspace_bytes": (C.c_size_t, [_i, _i, _i, _i]),
    "r2_proj_destripe_sort": (C.c_int, [_i, _i, _i, _fp, _i, _fp, _p, C.c_size_t, _p]),
    "r2_proj_destripe_mean": (C.c_int, [_i, _i, _i, _fp, _i, _fp, _fp, _p, C.c_size_t, _p]),
    "r2_gaussian_activate": (C.c_int, [_i, _fp, _fp, _fp, C.c_double, C.c_double, _fp, _fp, _fp, _p]),
    "r2_gaussian_adam_step": (C.c_int, [_i, _p, _p, _p, _p, _p, _p, _p, C.c_double, C.c_double, _fp, _fp, _fp, _p]),
    "r2_profile_enable": (None, [C.c_ulonglong]),
    "r2_profile_stage_count": (C.c_int, []),
    "r2_profile_stage_name": (C.c_char_p, [_i]),
    "r2_profile_read": (C.c_int, [C.POINTER(C.c_double), C.POINTER(C.c_longlong), _i]),
    "r2_sync_wait_stats": (C.c_int, [C.POINTER(C.c_double), C.POINTER(C.c_longlong), _i]),
    "r2_depth_hint_control": (None, [_i]),
    "r2_tile_first_control": (None, [_i]),
    "r2_profile_host": (C.c_int, [C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_longlong), _i]),
    "r2_raster_state_offset": (C.c_longlong, [_i, _i, C.c_longlong, _i, _i, C.POINTER(C.c_int)]),
    "r2_voxel_state_offset": (C.c_longlong, [_i, _i, C.c_longlong, _i, _i, _i, C.POINTER(C.c_int)]),
}

_lib = None


class R2HipError(RuntimeError):
    pass


def lib():
    """Load libr2hip.so once; raise loudly when it is absent (no CPU fallback exists)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise R2HipError(
                "libr2hip.so not found at %s -- the HIP extension is required (no fallback). "
                "Run `python -m r2_gaussian_amd.build`." % LIB_PATH)
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in _SIGNATURES.items():
            fn = getattr(L, name)   # AttributeError if a declared symbol is not exported
            fn.restype = res
            fn.argtypes = args
        if L.r2_abi_version() != R2_ABI_VERSION:
            raise R2HipError("libr2hip.so ABI %d != expected %d" % (L.r2_abi_version(), R2_ABI_VERSION))
        _lib = L
    return _lib


def exported_symbols():
    return sorted(_SIGNATURES)


def check(rc, what):
    if rc < 0:
        msg = lib().r2_last_error()
        raise R2HipError("%s failed (code %d): %s" % (what, rc, msg.decode() if msg else ""))
    return rc


def stage_names():
    L = lib()
    return [L.r2_profile_stage_name(i).decode() for i in range(L.r2_profile_stage_count())]


def profile_enable(stages=None):
    """Enable HIP-event timing for the named stages (None = all, [] = off)."""
    names = stage_names()
    if stages is None:
        mask = (1 << len(names)) - 1
    else:
        mask = 0
        for s in stages:
            mask |= 1 << names.index(s)
    lib().r2_profile_enable(mask)


def path_stats(reset=False):
    """-> {name: count} of the chain counters (csrc/dispatch.hpp): which chain every forward took and why."""
    L = lib()
    n = L.r2_path_stat_count()
    buf = (C.c_longlong * n)()
    L.r2_path_stats(buf, n, int(reset))
    return {L.r2_path_stat_name(i).decode(): int(buf[i]) for i in range(n)}


def sync_wait_stats(reset=True):
    """-> (total microseconds the host busy-waited for num_rendered, number of waits)."""
    us, n = C.c_double(0.0), C.c_longlong(0)
    lib().r2_sync_wait_stats(C.byref(us), C.byref(n), int(reset))
    return us.value, n.value


def profile_host(reset=True):
    """-> (host microseconds per forward before its synchronisation wait, after it, number of forwards)."""
    a, b, n = C.c_double(0.0), C.c_double(0.0), C.c_longlong(0)
    lib().r2_profile_host(C.byref(a), C.byref(b), C.byref(n), int(reset))
    return a.value / max(n.value, 1), b.value / max(n.value, 1), n.value


def profile_read(reset=True):
    """-> {stage: (total_ms, launches)} for stages that ran."""
    L = lib()
    n = L.r2_profile_stage_count()
    ms = (C.c_double * n)()
    cnt = (C.c_longlong * n)()
    L.r2_profile_read(ms, cnt, int(reset))
    names = stage_names()
    return {names[i]: (ms[i], cnt[i]) for i in range(n) if cnt[i] > 0}
