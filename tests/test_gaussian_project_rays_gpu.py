"""GPU: the exact Gaussian projector's gradient in its rays (r2_project_gaussians_rays_backward, csrc/gaussian_project_rays_bwd.hip;
autograd through r2_gaussian_amd.gaussian_projector.project_gaussians_rays) against the float64 restatement of its contract
(tests/gaussian_project_rays_ref.py), and r2_gaussian_amd.geometry.refine_geometry against the same loop on the host.

Tolerance: 4 x e32 x sum |pair contributions| per component of dL/drays, e32 being the measured error of the float32
restatement against float64 for that scene (tests/golden/gaussian_project_rays/e32.json; the factor 4 covers the device's
expf / sqrt / division against numpy's and the different association of the sums), plus the float32 underflow floor of the
reference module.  Bracket: the contract lets a pair with q > 32 be summed or skipped, so the kernel must lie between the
float64 sums cut at q <= 32 and the float64 sums of every pair, each widened by the tolerance, at every one of the V x 12
components; none is excluded.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import gaussian_project_rays_ref as Q

pytestmark = pytest.mark.gpu

E32 = Q.load_e32()
GUARD = 16          # guard words on either side of every buffer the C ABI writes
SENTINEL = -7.25


def _leaves(cloud, dev, grad=False):
    return [torch.from_numpy(a).to(dev).requires_grad_(grad) for a in cloud]


def _run(sc, dev, rays_grad=True, cloud_grad=False, rays=None):
    """project_gaussians_rays and loss = sum(G * image) backwards -> (image, rays leaf, cloud leaves)."""
    from r2_gaussian_amd.gaussian_projector import project_gaussians_rays
    rays = torch.from_numpy(sc["rays"] if rays is None else rays).to(dev).requires_grad_(rays_grad)
    leaves = _leaves(sc["cloud"], dev, cloud_grad)
    img = project_gaussians_rays(rays, sc["cone"], sc["H"], sc["W"], *leaves, scale_modifier=sc["mod"])
    if rays_grad or cloud_grad:
        G = torch.from_numpy(sc["G"][:rays.shape[0]]).to(dev)
        (img * G).sum().backward()
    return img.detach(), rays, leaves


@pytest.mark.parametrize("name", Q.SCENES)
def test_ray_gradient_vs_float64(gpu, name):
    """rays.grad (autograd end to end) inside the float64 bracket on every scene of the projector's tests -- P in {1, 7, 300},
    detectors 8x8, 17x23, 70x50, V in {1, 3}, the edge scenes -- and on `wide` (260 x 264: 289 tile partials per view)."""
    r = Q.reference(name)
    _, rays, _ = _run(r["scene"], gpu)
    assert rays.grad is not None and rays.grad.shape == rays.shape and rays.grad.dtype == torch.float32
    got = rays.grad.cpu().numpy().astype(np.float64)
    a, b = r["lo"]["grad"], r["hi"]["grad"]
    tol = 4.0 * E32[name] * r["hi"]["gabs"] + Q.FLOOR
    lo, hi = np.minimum(a, b) - tol, np.maximum(a, b) + tol
    worst = float(np.max(np.maximum(lo - got, got - hi) / tol))
    print("%s d rays: worst excess over the bracket in units of the tolerance %.3f (1 + this <= 1 passes)" % (name, worst))
    bad = (got < lo) | (got > hi) | ~np.isfinite(got)
    assert not bad.any(), "%s: %d of %d outside the bracket, worst excess %.3g tolerances" % (name, int(bad.sum()), bad.size, worst)


@pytest.mark.parametrize("beam", ["cone", "parallel"])
def test_other_outputs_unchanged_views_independent_calls_reproducible(gpu, beam):
    """The image and the four parameter gradients of a call whose rays require grad are the bits of one whose rays do not;
    views [a, b, c] give view b's twelve numbers bit-identically to [b] alone; two calls give the same bits."""
    sc = Q.scene(beam + "_p7")
    img, rays, leaves = _run(sc, gpu, cloud_grad=True)
    img0, rays0, leaves0 = _run(sc, gpu, rays_grad=False, cloud_grad=True)
    assert rays0.grad is None and torch.equal(img, img0)
    for a, b in zip(leaves, leaves0):
        assert torch.equal(a.grad, b.grad)
    _, one, _ = _run(dict(sc, G=sc["G"][1:2]), gpu, rays=sc["rays"][1:2].copy())
    _, three, _ = _run(dict(sc, G=sc["G"][[1, 0, 2]]), gpu, rays=sc["rays"][[1, 0, 2]].copy())
    assert torch.equal(one.grad[0], three.grad[0])
    _, again, _ = _run(sc, gpu)
    assert torch.equal(rays.grad, again.grad)


def test_host_rays_of_any_float_dtype_receive_the_gradient(gpu):
    """A float64 rays leaf on the host: its grad arrives there, in float64, with the values of the device float32 leaf."""
    from r2_gaussian_amd.gaussian_projector import project_gaussians_rays
    sc = Q.scene("cone_p7")
    _, dev_rays, _ = _run(sc, gpu)
    host = torch.from_numpy(sc["rays"]).double().requires_grad_(True)
    img = project_gaussians_rays(host, True, sc["H"], sc["W"], *_leaves(sc["cloud"], gpu))
    (img * torch.from_numpy(sc["G"]).to(gpu)).sum().backward()
    assert host.grad is not None and not host.grad.is_cuda and host.grad.dtype == torch.float64
    assert torch.equal(host.grad, dev_rays.grad.cpu().double())


def test_no_gaussians_gives_zeros(gpu):
    sc = Q.scene("cone_p7")
    e = lambda c: np.zeros((0, c), np.float32)
    _, rays, _ = _run(dict(sc, cloud=(e(3), e(1), e(3), e(4))), gpu)
    assert rays.grad.shape == (3, 12) and (rays.grad == 0).all()


@pytest.mark.parametrize("name", ["cone_offdet", "parallel_offdet", "cone_behind"])
def test_untouched_gaussians_change_no_bit(gpu, name):
    """A Gaussian that projects off the detector, or lies behind the cone source: dL/drays is bit-identical to the one of
    the cloud without it."""
    sc = Q.scene(name)
    _, rays, _ = _run(sc, gpu)
    keep = [i for i in range(sc["cloud"][0].shape[0]) if i not in sc["zero"]]
    _, rays2, _ = _run(dict(sc, cloud=tuple(a[keep] for a in sc["cloud"])), gpu)
    assert torch.isfinite(rays.grad).all() and (rays.grad != 0).any() and torch.equal(rays.grad, rays2.grad)


# ------------------------------------------------------------------------------------------------------ the C ABI itself
def _guarded(n, dev, dtype=torch.float32):
    """A buffer of n elements with GUARD sentinel elements on either side: (whole, middle view)."""
    whole = torch.full((n + 2 * GUARD,), SENTINEL if dtype == torch.float32 else 0xA5, dtype=dtype, device=dev)
    return whole, whole[GUARD:GUARD + n]


def _guards_intact(whole, n):
    fill = SENTINEL if whole.dtype == torch.float32 else 0xA5
    return bool((whole[:GUARD] == fill).all()) and bool((whole[GUARD + n:] == fill).all())


def _abi(sc, dev, ws_bytes=None, null_ws=False):
    """r2_project_gaussians_rays_backward through ctypes, dL_drays and the workspace between guard words.
    -> (rc, dL_drays [V,12], the workspace's middle, True when every guard survived)."""
    from r2_gaussian_amd import _lib
    L = _lib.lib()
    x, d, s, r = _leaves(sc["cloud"], dev)
    rays = torch.from_numpy(sc["rays"]).to(dev)
    G = torch.from_numpy(sc["G"]).to(dev)
    V, H, W, P = rays.shape[0], sc["H"], sc["W"], x.shape[0]
    need = int(L.r2_project_gaussians_rays_backward_workspace_bytes(V, H, W))
    assert need == 48 * V * ((H + 15) // 16) * ((W + 15) // 16)
    nws = need if ws_bytes is None else ws_bytes
    out, ws = _guarded(12 * V, dev), _guarded(nws, dev, torch.uint8)
    rc = L.r2_project_gaussians_rays_backward(V, H, W, rays.data_ptr(), int(sc["cone"]), P, x.data_ptr(), d.data_ptr(),
                                              s.data_ptr(), float(sc["mod"]), r.data_ptr(), G.data_ptr(), out[1].data_ptr(),
                                              None if null_ws else ws[1].data_ptr(), C.c_size_t(1 << 20 if null_ws else nws),
                                              torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize(dev)
    intact = _guards_intact(out[0], 12 * V) and _guards_intact(ws[0], nws)
    return rc, out[1].clone().reshape(V, 12), ws[1].clone(), intact


@pytest.mark.parametrize("name", ["cone_p7", "parallel_p300", "cone_wide"])
def test_guard_words_survive_and_autograd_is_the_c_abi(gpu, name):
    sc = Q.scene(name)
    rc, grad, _, intact = _abi(sc, gpu)
    assert rc == 0 and intact
    _, rays, _ = _run(sc, gpu)
    assert torch.equal(grad, rays.grad)


def test_null_or_short_workspace_is_refused(gpu):
    from r2_gaussian_amd import _lib
    sc = Q.scene("cone_p7")   # 3 views of 2 x 2 tiles: 576 bytes
    for kw in (dict(ws_bytes=575), dict(null_ws=True)):
        rc, grad, ws, intact = _abi(sc, gpu, **kw)
        assert rc == _lib.R2_ERR_INVALID and intact
        msg = _lib.lib().r2_last_error().decode()
        assert "workspace" in msg and "576" in msg
        assert (grad == SENTINEL).all() and (ws == 0xA5).all()   # nothing was launched


# ------------------------------------------------------------------------------------------------------ the refinement
def test_refinement_follows_the_host_loop(gpu):
    """refine_geometry on cone_p7's geometry, the projections measured with the detector shifted by 1.5 pixels, K steps from
    offDetector = 0 (tests/gaussian_project_rays_ref.py: REFINE_*).  The reference module runs the same loop on the host in
    float64 and in float32 (tests/golden/gaussian_project_rays/refine.json; the CPU tests re-measure it and check that the
    float64 loop ends below half its initial offset error).  The GPU's final offDetector must lie within
    4 x max |float32 loop - float64 loop| of the float64 loop's, in the maximum norm over the two parameters."""
    from r2_gaussian_amd.geometry import refine_geometry
    gold = Q.load_refine()
    st = Q.refine_setup()
    projs = torch.from_numpy(st["projs"]).to(gpu)
    start = {"offDetector": torch.zeros(2, dtype=torch.float64, device=gpu)}
    got, hist = refine_geometry(projs, _leaves(st["cloud"], gpu), Q.refine_rays_fn(st, gpu), start, gold["K"], gold["lr"])
    assert (start["offDetector"] == 0).all() and hist.shape == (gold["K"],) and hist.is_cuda
    p = got["offDetector"].cpu().numpy()
    dist, tol = float(np.abs(p - np.asarray(gold["final64"])).max()), 4.0 * gold["f32_minus_f64"]
    print("refinement: offDetector %s, float64 loop %s, distance %.3e, tolerance %.3e; loss %.3e -> %.3e (float64 loop %.3e -> %.3e)"
          % (p, gold["final64"], dist, tol, float(hist[0]), float(hist[-1]), gold["initial_loss64"], gold["final_loss64"]))
    assert dist <= tol


def test_argument_errors(gpu):
    from r2_gaussian_amd import _lib
    from r2_gaussian_amd.gaussian_projector import project_gaussians_rays
    from r2_gaussian_amd.geometry import refine_geometry
    sc = Q.scene("cone_p7")
    x, d, s, r = _leaves(sc["cloud"], gpu)
    rays = torch.from_numpy(sc["rays"]).to(gpu).requires_grad_(True)
    with pytest.raises(ValueError):
        project_gaussians_rays(rays, True, 17, 23, x.cpu(), d, s, r)
    with pytest.raises(ValueError):
        project_gaussians_rays(rays[:, :11], True, 17, 23, x, d, s, r)
    with pytest.raises(ValueError):
        refine_geometry(torch.zeros(3, 17, 23), (x, d, s, r), lambda p: rays, {}, 1, 0.1)
    with pytest.raises(ValueError):
        refine_geometry(torch.zeros(3, 17, 23, device=gpu), (x, d, s, r), lambda p: rays, {}, 1, 0.1, loss="huber")
    L = _lib.lib()
    z = torch.zeros(16, device=gpu)
    rc = L.r2_project_gaussians_rays_backward(1, 8, 8, z.data_ptr(), 1, 1, z.data_ptr(), z.data_ptr(), z.data_ptr(), 1.0,
                                              z.data_ptr(), z.data_ptr(), None, z.data_ptr(), C.c_size_t(64), None)
    assert rc == _lib.R2_ERR_INVALID and "invalid argument" in L.r2_last_error().decode()
