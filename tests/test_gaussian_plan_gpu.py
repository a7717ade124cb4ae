"""GPU: projection plans (csrc/gaussian_plan.hip, the list round of csrc/gaussian_skeleton.hpp and the *_planned entries of
the five pixel-major operators of the exact projector; include/r2hip.h, "projection plans").

A planned operator stages the Gaussians of its tile's list as the unplanned one stages its hits and a pixel adds the same
pairs in the same order, so EVERY comparison here is torch.equal: no tolerance appears anywhere.  A planned output that
differs from its unplanned twin in one bit is a bug in the lists or in the staging, never a rounding matter.
"""
import numpy as np
import pytest
import torch

from tests import gaussian_fisher_ref as RFI
from tests import gaussian_project_ref as RP
from tests import gaussian_tangent_ref as R

pytestmark = pytest.mark.gpu

GUARD = 16
SENTINEL = -7.25
_SCENES = {}


def _scene(name):
    if name not in _SCENES:
        _SCENES[name] = RP.scene(name)
    return _SCENES[name]


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _groups(d, dev):
    return tuple(_t(d[k], dev) for k in R.GROUPS)


def _setup(sc, dev, cloud=None, rays=None):
    """-> (rays tensor, the four cloud tensors, the plan built from exactly these)."""
    from r2_gaussian_amd.gaussian_projector import plan_projection_rays
    rays = _t(sc["rays"] if rays is None else rays, dev)
    cloud = [_t(a, dev) for a in (sc["cloud"] if cloud is None else cloud)]
    return rays, cloud, plan_projection_rays(rays, sc["cone"], sc["H"], sc["W"], *cloud, scale_modifier=sc["mod"])


def _forward(sc, rays, cloud, plan=None, out=None):
    from r2_gaussian_amd.gaussian_projector import project_gaussians_rays
    return project_gaussians_rays(rays, sc["cone"], sc["H"], sc["W"], *cloud, scale_modifier=sc["mod"], out=out, plan=plan)


def _jvp(sc, rays, cloud, tan, plan=None):
    from r2_gaussian_amd.gaussian_projector import project_gaussians_rays_jvp
    return project_gaussians_rays_jvp(rays, sc["cone"], sc["H"], sc["W"], *cloud, tangents=tan, scale_modifier=sc["mod"], plan=plan)


def _jac(sc, rays, cloud, plan=None):
    from r2_gaussian_amd.geometry import ray_jacobian
    return ray_jacobian(rays, sc["cone"], sc["H"], sc["W"], *cloud, scale_modifier=sc["mod"], plan=plan)


def _tiles(sc):
    return (sc["H"] + 15) // 16, (sc["W"] + 15) // 16


def _lists(plan):
    """-> the plan's lists as a list of numpy arrays, one per (view, tile)."""
    off, ids = (t.cpu().numpy() for t in plan.lists())
    return [ids[off[k]:off[k + 1]] for k in range(off.shape[0] - 1)]


# ------------------------------------------------------------------------------------------------------ 1: bit identity
@pytest.mark.parametrize("name", RP.SCENES)
def test_planned_operators_are_bit_identical(gpu, name):
    """The forward, the four parameter gradients and the ray gradient through autograd (G = the scene's), the JVP with the
    tangent of the tangent tests, the projection variance and the ray Jacobian, planned against unplanned."""
    from r2_gaussian_amd.uncertainty import projection_variance_rays
    sc = _scene(name)
    rays, cloud, plan = _setup(sc, gpu)
    rays.requires_grad_(True)
    for t in cloud:
        t.requires_grad_(True)
    G = _t(sc["G"], gpu)
    img_p, img_u = _forward(sc, rays, cloud, plan), _forward(sc, rays, cloud)
    assert torch.equal(img_p, img_u)
    grads_p = torch.autograd.grad(img_p, cloud + [rays], G)
    grads_u = torch.autograd.grad(img_u, cloud + [rays], G)
    for what, a, b in zip(R.GROUPS + ("rays",), grads_p, grads_u):
        assert torch.equal(a, b), (name, what)
    P = cloud[0].shape[0]
    tan = _groups(R.scene_tangents(P), gpu)
    assert torch.equal(_jvp(sc, rays, cloud, tan, plan), _jvp(sc, rays, cloud, tan))
    var = _groups(RFI.scene_variances(P), gpu)
    args = (rays, sc["cone"], sc["H"], sc["W"], *cloud, var)
    assert torch.equal(projection_variance_rays(*args, scale_modifier=sc["mod"], plan=plan),
                       projection_variance_rays(*args, scale_modifier=sc["mod"]))
    assert torch.equal(_jac(sc, rays, cloud, plan), _jac(sc, rays, cloud))
    if not sc["zero"] or P > len(sc["zero"]):
        assert (img_p != 0).any()


def test_view_entry_points_take_a_plan_of_views(gpu):
    """plan_projection on views serves project_gaussians, project_gaussians_jvp and projection_variance; other views raise."""
    from r2_gaussian_amd.gaussian_projector import plan_projection, project_gaussians, project_gaussians_jvp
    from r2_gaussian_amd.uncertainty import projection_variance
    sc = _scene("cone_p300")
    cloud = [_t(a, gpu) for a in sc["cloud"]]
    plan = plan_projection(sc["views"], *cloud)
    assert torch.equal(project_gaussians(sc["views"], *cloud, plan=plan), project_gaussians(sc["views"], *cloud))
    tan = _groups(R.scene_tangents(300), gpu)
    assert torch.equal(project_gaussians_jvp(sc["views"], *cloud, tangents=tan, plan=plan),
                       project_gaussians_jvp(sc["views"], *cloud, tangents=tan))
    var = _groups(RFI.scene_variances(300), gpu)
    assert torch.equal(projection_variance(sc["views"], *cloud, var, plan=plan), projection_variance(sc["views"], *cloud, var))
    with pytest.raises(ValueError, match="views"):
        project_gaussians(sc["views"][:2], *cloud, plan=plan)


# ------------------------------------------------------------------------------------------------------ 2: the batch edge
@pytest.mark.parametrize("P", [255, 256, 257])
def test_lists_of_one_batch_minus_one_one_batch_and_one_more(gpu, P):
    sc = _scene("cone_stack300")
    rays, cloud, plan = _setup(sc, gpu, cloud=tuple(a[:P] for a in sc["cloud"]))
    assert max(len(l) for l in _lists(plan)) == P   # every Gaussian of the stack lies on the one tile
    assert torch.equal(_forward(sc, rays, cloud, plan), _forward(sc, rays, cloud))
    tan = _groups({k: v[:P] for k, v in R.scene_tangents(300).items()}, gpu)
    assert torch.equal(_jvp(sc, rays, cloud, tan, plan), _jvp(sc, rays, cloud, tan))


# ------------------------------------------------------------------------------------------------------ 3: empty lists
def _corner_scene(beam):
    """A 40 x 40 detector (9 tiles) and three Gaussians of sigma 0.01 on and next to the ray of pixel (2, 2)."""
    from r2_gaussian_amd import projector
    views = RP._views(beam, 1, (40, 40))
    rays = projector.ray_params(views, (1.0, 1.0, 1.0), (0.0, 0.0, 0.0), (1, 1, 1))
    a, p00, pu, pv = (rays[0, 3 * k:3 * k + 3].astype(np.float64) for k in range(4))
    pix = p00 + 2.0 * pu + 2.0 * pv
    on_ray = a + 5.0 * (pix - a) if beam == "cone" else pix + 0.0 * a   # cone: |pix - a| is about 1, the source 5 from the origin
    xyz = np.stack([on_ray, on_ray + 0.004, on_ray - 0.003]).astype(np.float32)
    cloud = (xyz, np.full((3, 1), 0.7, np.float32), np.full((3, 3), 0.01, np.float32),
             np.tile(np.array([[1.0, 0.0, 0.0, 0.0]], np.float32), (3, 1)))
    return {"views": views, "rays": rays, "cone": beam == "cone", "H": 40, "W": 40, "cloud": cloud, "mod": 1.0}


@pytest.mark.parametrize("beam", ["cone", "parallel"])
def test_tiles_with_empty_lists_write_their_zeros(gpu, beam):
    sc = _corner_scene(beam)
    rays, cloud, plan = _setup(sc, gpu)
    sizes = [len(l) for l in _lists(plan)]
    assert len(sizes) == 9 and min(sizes) == 0 and max(sizes) == 3, sizes
    out = torch.full((1, 40, 40), float("nan"), device=gpu)
    got = _forward(sc, rays, cloud, plan, out=out)
    assert not torch.isnan(got).any() and torch.equal(got, _forward(sc, rays, cloud)) and (got != 0).any()
    assert (got[0, 16:, 16:] == 0).all()
    jac = _jac(sc, rays, cloud, plan)
    assert not torch.isnan(jac).any() and torch.equal(jac, _jac(sc, rays, cloud)) and (jac != 0).any()
    # the entry itself on a NaN buffer: ray_jacobian allocates its own output
    from r2_gaussian_amd import _lib
    buf = torch.full((1, 6, 40, 40), float("nan"), device=gpu)
    x, d, s, q = cloud
    rc = _lib.lib().r2_project_gaussians_ray_jacobian_planned(1, 40, 40, rays.data_ptr(), int(sc["cone"]), 3, x.data_ptr(),
                                                              d.data_ptr(), s.data_ptr(), 1.0, q.data_ptr(), buf.data_ptr(),
                                                              plan.offsets.data_ptr(), plan.ids.data_ptr(), plan.ids.numel(),
                                                              torch.cuda.current_stream(gpu).cuda_stream)
    torch.cuda.synchronize(gpu)
    assert rc == 0 and torch.equal(buf, jac)


# ------------------------------------------------------------------------------------------------------ 4: plan structure
@pytest.mark.parametrize("name", ["cone_p300", "parallel_p300", "cone_offdet", "cone_cover"])
def test_plan_structure(gpu, name):
    sc = _scene(name)
    rays, cloud, plan = _setup(sc, gpu)
    V, P = rays.shape[0], cloud[0].shape[0]
    Ty, Tx = _tiles(sc)
    off, ids = plan.lists()
    assert off.dtype == torch.int64 and ids.dtype == torch.int32 and off.is_cuda and ids.is_cuda
    assert (plan.V, plan.H, plan.W, plan.cone, plan.P, plan.scale_modifier) == (V, sc["H"], sc["W"], sc["cone"], P, sc["mod"])
    off = off.cpu().numpy()
    assert off.shape == (V * Ty * Tx + 1,) and off[0] == 0 and (np.diff(off) >= 0).all()
    assert off[-1] == plan.instances == ids.numel() and plan.instances > 0
    lists = _lists(plan)
    for l in lists:
        assert (np.diff(l) > 0).all() and (l >= 0).all() and (l < P).all()
    if name == "cone_offdet":
        assert sc["zero"] == [1] and not any((l == 1).any() for l in lists)
    if name == "cone_cover":
        assert all((l == 1).any() for l in lists)


# ------------------------------------------------------------------------------------------------------ 5: deterministic, per view
def test_building_twice_gives_the_same_bytes_and_views_do_not_mix(gpu):
    from r2_gaussian_amd import projector
    sc = _scene("cone_p300")
    _, _, one = _setup(sc, gpu)
    _, _, two = _setup(sc, gpu)
    assert torch.equal(one.offsets, two.offsets) and torch.equal(one.ids, two.ids)
    extra = projector.ray_params(RFI.candidate_views("cone_p300", (1.2,)), (1.0, 1.0, 1.0), (0.0, 0.0, 0.0), (1, 1, 1))
    _, _, more = _setup(sc, gpu, rays=np.concatenate([sc["rays"], extra], 0))
    n = one.offsets.numel()
    assert more.offsets.numel() > n and torch.equal(more.offsets[:n], one.offsets)
    assert torch.equal(more.ids[:one.instances], one.ids) and more.instances > one.instances


# ------------------------------------------------------------------------------------------------------ 6: lists drive the kernel
def _guarded(n, dev, fill=SENTINEL):
    whole = torch.full((n + 2 * GUARD,), fill, dtype=torch.float32, device=dev)
    return whole, whole[GUARD:GUARD + n]


def _intact(whole, n):
    return bool((whole[:GUARD] == SENTINEL).all()) and bool((whole[GUARD + n:] == SENTINEL).all())


def _planned_forward(L, sc, rays, cloud, out, offsets, ids, capacity, dev):
    x, d, s, q = cloud
    rc = L.r2_project_gaussians_planned(rays.shape[0], sc["H"], sc["W"], rays.data_ptr(), int(sc["cone"]), x.shape[0], x.data_ptr(),
                                        d.data_ptr(), s.data_ptr(), float(sc["mod"]), q.data_ptr(), out.data_ptr(),
                                        None if offsets is None else offsets.data_ptr(), None if ids is None else ids.data_ptr(),
                                        capacity, torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize(dev)
    return rc


def test_the_lists_drive_the_kernel(gpu):
    from r2_gaussian_amd import _lib
    L = _lib.lib()
    sc = _scene("cone_p7")
    rays, cloud, plan = _setup(sc, gpu)
    V, H, W = rays.shape[0], sc["H"], sc["W"]
    Ty, Tx = _tiles(sc)
    T, n = Ty * Tx, V * H * W
    # every list empty: exact zeros over a NaN buffer, the guard words intact
    whole, out = _guarded(n, gpu)
    out.fill_(float("nan"))
    empty = torch.zeros((V * T + 1,), dtype=torch.int64, device=gpu)
    assert _planned_forward(L, sc, rays, cloud, out, empty, None, 0, gpu) == 0
    assert (out == 0).all() and not torch.signbit(out).any() and _intact(whole, n)
    # hand-made lists: Gaussian 2 alone, in every tile of view 0
    off = torch.tensor(list(range(T + 1)) + [T] * (V * T - T), dtype=torch.int64, device=gpu)
    ids = torch.full((T,), 2, dtype=torch.int32, device=gpu)
    whole, out = _guarded(n, gpu)
    assert _planned_forward(L, sc, rays, cloud, out, off, ids, T, gpu) == 0 and _intact(whole, n)
    alone = [t[2:3].contiguous() for t in cloud]
    want = _forward(sc, rays[:1].contiguous(), alone)
    out = out.reshape(V, H, W)
    assert torch.equal(out[:1], want) and (want != 0).any() and (out[1:] == 0).all()
    # the true lists and a capacity that ends in the middle of them: the tiles whose lists lie below it are unchanged
    true = _forward(sc, rays, cloud)
    offs = plan.offsets.cpu().numpy()
    k = int(np.searchsorted(offs, plan.instances // 2, side="right")) - 1   # list k is the last that starts at or below it
    cap = int(offs[k])
    assert 0 < cap < plan.instances and k >= 1
    whole, out = _guarded(n, gpu)
    assert _planned_forward(L, sc, rays, cloud, out, plan.offsets, plan.ids, cap, gpu) == 0 and _intact(whole, n)
    out = out.reshape(V, H, W)
    for j in range(k):   # lists 0 .. k - 1 end at or below the capacity
        v, ty, tx = j // T, (j % T) // Tx, j % Tx
        tile = (v, slice(16 * ty, 16 * ty + 16), slice(16 * tx, 16 * tx + 16))
        assert torch.equal(out[tile], true[tile]), j
    assert torch.isfinite(out).all()


# ------------------------------------------------------------------------------------------------------ 7: P = 0 and P = 1
def test_no_gaussians_and_one(gpu):
    sc = _scene("cone_p7")
    rays, cloud, plan = _setup(sc, gpu, cloud=tuple(a[:0] for a in sc["cloud"]))
    assert plan.instances == 0 and plan.ids.numel() == 0 and (plan.offsets == 0).all() and plan.P == 0
    out = torch.full((rays.shape[0], sc["H"], sc["W"]), float("nan"), device=gpu)
    assert (_forward(sc, rays, cloud, plan, out=out) == 0).all()
    assert (_jac(sc, rays, cloud, plan) == 0).all()
    rays, cloud, plan = _setup(sc, gpu, cloud=tuple(a[:1] for a in sc["cloud"]))
    assert plan.instances > 0 and (plan.ids == 0).all()
    img = _forward(sc, rays, cloud, plan)
    assert torch.equal(img, _forward(sc, rays, cloud)) and (img != 0).any()


# ------------------------------------------------------------------------------------------------------ 8: staleness
def test_a_stale_plan_is_an_error(gpu):
    from r2_gaussian_amd.gaussian_projector import project_gaussians_rays
    sc = _scene("cone_p7")
    rays, cloud, plan = _setup(sc, gpu)
    H, W = sc["H"], sc["W"]
    project_gaussians_rays(rays, True, H, W, *cloud, plan=plan)
    with pytest.raises(ValueError, match="rays"):
        project_gaussians_rays(rays.clone(), True, H, W, *cloud, plan=plan)
    with pytest.raises(ValueError, match="H changed"):
        project_gaussians_rays(rays, True, H + 1, W, *cloud, plan=plan)
    with pytest.raises(ValueError, match="cone"):
        project_gaussians_rays(rays, False, H, W, *cloud, plan=plan)
    with pytest.raises(ValueError, match="scale_modifier"):
        project_gaussians_rays(rays, True, H, W, *cloud, scale_modifier=0.5, plan=plan)
    fewer = [t[:5].contiguous() for t in cloud]
    with pytest.raises(ValueError, match="xyz"):
        project_gaussians_rays(rays, True, H, W, *fewer, plan=plan)
    with pytest.raises(ValueError):
        project_gaussians_rays(rays, True, H, W, *cloud, plan="a plan")
    cloud[0].add_(0)
    with pytest.raises(ValueError, match="xyz"):
        project_gaussians_rays(rays, True, H, W, *cloud, plan=plan)
    with pytest.raises(ValueError, match="xyz"):
        _jvp(sc, rays, cloud, _groups(R.scene_tangents(7), gpu), plan)
    with pytest.raises(ValueError, match="xyz"):
        _jac(sc, rays, cloud, plan)


# ------------------------------------------------------------------------------------------------------ 9: the solvers
def test_planned_solvers_give_the_same_bits(gpu):
    from r2_gaussian_amd.gauss_newton import gauss_newton_step, normal_matvec, refine_cloud
    sc = _scene("cone_p300")
    rays, cloud = _t(sc["rays"], gpu), [_t(a, gpu) for a in sc["cloud"]]
    tan = _groups(R.scene_tangents(300), gpu)
    w = _t(RFI.scene_weights(rays.shape[0], sc["H"], sc["W"]), gpu)
    a = normal_matvec(rays, True, sc["H"], sc["W"], cloud, tan, weights=w, damping=0.5, planned=True)
    b = normal_matvec(rays, True, sc["H"], sc["W"], cloud, tan, weights=w, damping=0.5, planned=False)
    assert all(torch.equal(x, y) for x, y in zip(a, b)) and all((x != 0).any() for x in a)
    gold = R.load_gauss_newton()
    st = R.gauss_newton_setup()
    projs, rays, start = _t(st["projs"], gpu), _t(st["rays"], gpu), [_t(a, gpu) for a in st["start"]]
    (ca, la), (cb, lb) = (gauss_newton_step(rays, True, st["H"], st["W"], start, projs, gold["cg_iters"], gold["damping"], planned=p)
                          for p in (True, False))
    assert torch.equal(la, lb) and all(torch.equal(x, y) for x, y in zip(ca, cb))
    (ca, ha), (cb, hb) = (refine_cloud(rays, projs, start, gold["steps"], gold["cg_iters"], gold["damping"], cone=True,
                                       max_log_step=gold["max_log_step"], planned=p) for p in (True, False))
    assert torch.equal(ha, hb) and all(torch.equal(x, y) for x, y in zip(ca, cb))
    assert float(ha[-1]) < float(ha[0])


# ------------------------------------------------------------------------------------------------------ 10: C argument errors
def test_c_argument_errors_write_nothing(gpu):
    from r2_gaussian_amd import _lib
    L = _lib.lib()
    stream = torch.cuda.current_stream(gpu).cuda_stream
    sc = _scene("cone_p7")
    rays, cloud, plan = _setup(sc, gpu)
    x, d, s, q = cloud
    V, H, W, P = rays.shape[0], sc["H"], sc["W"], 7
    n = V * H * W
    for what, off, ids, cap in (("NULL offsets", None, plan.ids, plan.instances), ("NULL ids", plan.offsets, None, plan.instances)):
        whole, out = _guarded(n, gpu)
        rc = _planned_forward(L, sc, rays, cloud, out, off, ids, cap, gpu)
        assert rc == _lib.R2_ERR_INVALID and "r2_project_gaussians_planned" in L.r2_last_error().decode(), what
        assert (whole == SENTINEL).all(), what
    head = (V, H, W, rays.data_ptr(), 1, P, x.data_ptr(), d.data_ptr(), s.data_ptr(), 1.0, q.data_ptr())
    need = int(L.r2_project_gaussians_plan_workspace_bytes(V, H, W, P))
    ws = torch.zeros((need,), dtype=torch.uint8, device=gpu)
    offsets = torch.full((plan.offsets.numel(),), -3, dtype=torch.int64, device=gpu)
    rc = L.r2_project_gaussians_plan_count(*head, offsets.data_ptr(), ws.data_ptr(), need - 1, stream)
    msg = L.r2_last_error().decode()
    torch.cuda.synchronize(gpu)
    assert rc == _lib.R2_ERR_INVALID and "r2_project_gaussians_plan_count" in msg and "r2_project_gaussians_plan_workspace_bytes" in msg
    assert (offsets == -3).all() and (ws == 0).all()
    ids = torch.full((plan.instances,), -3, dtype=torch.int32, device=gpu)
    for what, off_p, ids_p, size in (("small workspace", plan.offsets.data_ptr(), ids.data_ptr(), need - 1),
                                     ("NULL offsets", None, ids.data_ptr(), need), ("NULL ids", plan.offsets.data_ptr(), None, need)):
        rc = L.r2_project_gaussians_plan_fill(*head, off_p, ids_p, plan.instances, ws.data_ptr(), size, stream)
        msg = L.r2_last_error().decode()
        torch.cuda.synchronize(gpu)
        assert rc == _lib.R2_ERR_INVALID and "r2_project_gaussians_plan_fill" in msg, what
        assert ("r2_project_gaussians_plan_workspace_bytes" in msg) == (what == "small workspace"), msg
        assert (ids == -3).all(), what
    G = torch.ones((n,), device=gpu)
    whole, grad = _guarded(V * 12, gpu)
    small = int(L.r2_project_gaussians_rays_backward_workspace_bytes(V, H, W)) - 1
    ws2 = torch.zeros((small + 1,), dtype=torch.uint8, device=gpu)
    rc = L.r2_project_gaussians_rays_backward_planned(*head, G.data_ptr(), grad.data_ptr(), ws2.data_ptr(), small,
                                                      plan.offsets.data_ptr(), plan.ids.data_ptr(), plan.instances, stream)
    msg = L.r2_last_error().decode()
    torch.cuda.synchronize(gpu)
    assert rc == _lib.R2_ERR_INVALID and "r2_project_gaussians_rays_backward_planned" in msg
    assert "r2_project_gaussians_rays_backward_workspace_bytes" in msg and (whole == SENTINEL).all() and (ws2 == 0).all()
