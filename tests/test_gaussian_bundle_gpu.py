"""GPU: the exact line integrals along caller-supplied rays (r2_gaussian_amd.gaussian_projector.integrate_rays;
csrc/gaussian_bundle.hip and its backward) against the float64 restatement of their contract (tests/gaussian_bundle_ref.py).

Tolerance: 4 x e32 x sum_g |term_g| per ray (and 4 x e32_k x sum_pairs |contribution| per gradient component), e32 being the
measured error of the float32 restatement against float64 for that scene (tests/golden/gaussian_bundle/e32.json; the factor 4
is DESIGN.md section 4's for this family: the device's expf / sqrtf / division against numpy's and the different association
of the sums), plus the float32 underflow floor of the reference module.  Bracket: a pair with q > 32 is summed only in the
sliver up to the cut, so the kernels must lie between the float64 sum cut at q <= 32 and the float64 sum of every pair, each
widened by the tolerance, at every ray and every gradient component; none is excluded.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import gaussian_bundle_ref as B
from tests import gaussian_project_rays_ref as RR
from tests import gaussian_project_ref as R

pytestmark = pytest.mark.gpu

E32 = B.load_e32()
GUARD = 16          # guard words on either side of every buffer the C ABI writes
SENTINEL = -7.25


def _leaves(cloud, dev, grad=False):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(dev).requires_grad_(grad) for a in cloud]


def _integrate(sc, dev, grad=False, sort=False):
    """-> (values, [xyz, density, scaling, rotation, origins, directions] leaves)."""
    from r2_gaussian_amd.gaussian_projector import integrate_rays
    leaves = _leaves(sc["cloud"], dev, grad)
    o = torch.from_numpy(sc["origins"]).to(dev).requires_grad_(grad)
    d = torch.from_numpy(sc["directions"]).to(dev).requires_grad_(grad)
    return integrate_rays(o, d, *leaves, scale_modifier=sc["mod"], half_line=sc["half_line"], sort=sort), leaves + [o, d]


def _grads(sc, dev, sort=False):
    val, leaves = _integrate(sc, dev, grad=True, sort=sort)
    G = torch.from_numpy(sc["G"]).to(dev).reshape(val.shape)
    return val.detach(), dict(zip(B.GRADS, torch.autograd.grad(val, leaves, G)))


def _bracket(got, a, b, tol, what):
    got = np.asarray(got, np.float64).reshape(a.shape)
    lo, hi = np.minimum(a, b) - tol, np.maximum(a, b) + tol
    bad = (got < lo) | (got > hi) | ~np.isfinite(got)
    worst = float(np.max(np.maximum(lo - got, got - hi) / np.maximum(tol, 1e-300))) if got.size else -1.0
    print("%s: worst excess over the bracket in units of the tolerance %.3f (1 + this <= 1 passes)" % (what, worst))
    assert not bad.any(), "%s: %d of %d outside the bracket, worst excess %.3g tolerances" % (what, int(bad.sum()), bad.size, worst)


def _check(r, e32, name, val, grads, groups=B.GRADS, factor=4.0):
    """val / grads inside the bracket of the reference r = {lo, hi} at factor x the e32 of one scene."""
    if val is not None:
        _bracket(val.cpu().numpy(), r["lo"]["val"], r["hi"]["val"], factor * e32["value"] * r["hi"]["abs"] + B.FLOOR, name + " value")
    for k in groups:
        tol = factor * e32[k] * r["hi"]["gabs"][k] + B.FLOOR
        _bracket(grads[k].cpu().numpy(), r["lo"]["grads"][k], r["hi"]["grads"][k], tol, name + " d" + k)


@pytest.mark.parametrize("name", B.SCENES)
def test_forward_and_backward_vs_float64(gpu, name):
    """Values and all six gradients (autograd end to end) inside the float64 bracket on every scene of the reference module:
    the pixel rays of a flat detector in both beams, scattered lines with |d| from 0.01 to 100, the block tails N = 1, 255,
    256, 257, 513, P = 700 (two full rounds of 256 and a partial one), P = 0, a curved detector, lines that miss the cloud
    box, half lines that start inside the cloud, cloud and rays 100 extents away, sigma = 5e-4 seen from six units away (at
    the origin and 100 extents away), raw quaternions of norm 0.3 .. 3, a nearly singular rotation (an infinite sphere),
    scale_modifier 0.5 and 2, non-finite and zero rows."""
    sc = B.reference(name)["scene"]
    val, grads = _grads(sc, gpu)
    assert val.shape == sc["origins"].shape[:-1] and val.dtype == torch.float32
    _check(B.reference(name), E32[name], name, val, grads)


@pytest.mark.parametrize("name", ["miss", "none", "bad"])
def test_exact_zeros(gpu, name):
    """Rays that miss the cloud box and P = 0: zeros everywhere.  `bad`: exact zeros for the gradients of the Gaussians with a
    NaN mean, an inf scale, a zero scale, and for the value and gradients of the rays with a NaN, an inf or no direction;
    everything finite; the values and ray gradients of the good rays are bit-identical to the call without the bad
    Gaussians."""
    sc = B.reference(name)["scene"]
    val, grads = _grads(sc, gpu)
    if name in ("miss", "none"):
        assert (val == 0).all()
        assert all((g == 0).all() for g in grads.values())
        return
    zg, zr = sc["zero_gaussians"], sc["zero_rays"]
    assert torch.isfinite(val).all() and all(torch.isfinite(g).all() for g in grads.values())
    assert (val[zr] == 0).all() and (grads["origins"][zr] == 0).all() and (grads["directions"][zr] == 0).all()
    for k in B.PARAMS:
        assert (grads[k][zg] == 0).all()
    keep = [i for i in range(sc["cloud"][0].shape[0]) if i not in zg]
    val2, grads2 = _grads(dict(sc, cloud=tuple(a[keep] for a in sc["cloud"])), gpu)
    assert torch.equal(val, val2) and (val != 0).sum() > 20
    assert torch.equal(grads["origins"], grads2["origins"]) and torch.equal(grads["directions"], grads2["directions"])
    for k in B.PARAMS:
        assert torch.equal(grads[k][keep], grads2[k])


def _far_rays(n, seed):
    """n rays 50 units and more away: half of them aimed through the cloud (they stretch the boxes of their blocks across it),
    half of them parallel to the x axis at |y| >= 40 (they miss the cloud box)."""
    g = np.random.RandomState(seed)
    u = g.randn(n, 3)
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    o = 50.0 * u * (1.0 + g.rand(n, 1))
    d = ((g.rand(n, 3) * 2 - 1) * 0.3 - o) * np.exp(g.uniform(-2, 2, (n, 1)))
    o[1::2, 1] = np.where(o[1::2, 1] >= 0, 40.0, -40.0) + o[1::2, 1]
    d[1::2] = (1.0, 0.0, 0.0)
    return o.astype(np.float32), d.astype(np.float32)


@pytest.mark.parametrize("name", ["scattered", "flat_cone", "flat_parallel"])
def test_a_ray_does_not_depend_on_the_other_rays(gpu, name):
    """The same rays under a fixed random permutation, and with 300 far-away rays interleaved: values and dL_drays per ray are
    bit-identical; sort=True gives the same bits too; the parameter gradients of the permuted call, whose sums associate
    differently, stay inside the bracket."""
    r = B.reference(name)
    sc = r["scene"]
    o, d = sc["origins"].reshape(-1, 3), sc["directions"].reshape(-1, 3)
    flat = dict(sc, origins=o, directions=d)
    v0, g0 = _grads(flat, gpu)
    N = o.shape[0]
    perm = np.random.RandomState(77).permutation(N)
    v1, g1 = _grads(dict(flat, origins=o[perm], directions=d[perm], G=sc["G"][perm]), gpu)
    pt = torch.from_numpy(perm).to(gpu)
    assert torch.equal(v1, v0[pt]) and torch.equal(g1["origins"], g0["origins"][pt]) and torch.equal(g1["directions"], g0["directions"][pt])
    _check(r, E32[name], name + " permuted", None, g1, groups=B.PARAMS)
    fo, fd = _far_rays(300, 78)
    where = np.sort(np.random.RandomState(79).permutation(N + 300)[:N])   # the slots the scene's rays keep, in order
    o2, d2, G2 = np.zeros((N + 300, 3), np.float32), np.zeros((N + 300, 3), np.float32), np.zeros(N + 300, np.float32)
    rest = np.setdiff1d(np.arange(N + 300), where)
    o2[where], d2[where], G2[where], o2[rest], d2[rest] = o, d, sc["G"], fo, fd
    v2, g2 = _grads(dict(flat, origins=o2, directions=d2, G=G2), gpu)
    wt = torch.from_numpy(where).to(gpu)
    assert torch.equal(v2[wt], v0) and torch.equal(g2["origins"][wt], g0["origins"]) and torch.equal(g2["directions"][wt], g0["directions"])
    assert (v2[torch.from_numpy(rest[1::2]).to(gpu)] == 0).all()
    if name == "scattered":
        assert (v2[torch.from_numpy(rest[0::2]).to(gpu)] != 0).sum() > 50   # the far rays through the cloud do sum
    v3, g3 = _grads(flat, gpu, sort=True)
    assert torch.equal(v3, v0) and torch.equal(g3["origins"], g0["origins"]) and torch.equal(g3["directions"], g0["directions"])
    _check(r, E32[name], name + " sorted", None, g3, groups=B.PARAMS)


def test_calls_are_reproducible(gpu):
    sc = B.scene("scattered")
    v1, g1 = _grads(sc, gpu)
    v2, g2 = _grads(sc, gpu)
    assert torch.equal(v1, v2)
    for k in B.GRADS:
        assert torch.equal(g1[k], g2[k]), k


@pytest.mark.parametrize("beam", ["cone", "parallel"])
def test_against_the_projector(gpu, beam):
    """integrate_rays(pixel_rays(rays), half_line=cone) and project_gaussians_rays on the same [V,12] both lie inside the
    float64 bracket of the flat scene, for the image and the four parameter gradients; dL_drays pushed through pixel_rays by
    autograd, and the projector's own [V,12] ray gradient, both lie inside the bracket of the projector's ray gradient
    (tests/gaussian_project_rays_ref.py, its e32)."""
    from r2_gaussian_amd import geometry
    from r2_gaussian_amd.gaussian_projector import integrate_rays, project_gaussians_rays
    name = "flat_" + beam
    r = B.reference(name)
    sc = r["scene"]
    pr = R.scene(beam + "_p300_small")
    H, W, cone = pr["H"], pr["W"], pr["cone"]
    G = torch.from_numpy(pr["G"]).to(gpu)
    out = {}
    for which in ("bundle", "projector"):
        leaves = _leaves(pr["cloud"], gpu, True)
        rays = torch.from_numpy(pr["rays"]).to(gpu).requires_grad_(True)
        if which == "bundle":
            o, d = geometry.pixel_rays(rays, cone, H, W)
            assert np.array_equal(o.detach().cpu().numpy(), sc["origins"]) and np.array_equal(d.detach().cpu().numpy(), sc["directions"])
            img = integrate_rays(o, d, *leaves, scale_modifier=pr["mod"], half_line=cone)
        else:
            img = project_gaussians_rays(rays, cone, H, W, *leaves, scale_modifier=pr["mod"])
        assert img.shape == (1, H, W)
        grads = torch.autograd.grad(img, leaves + [rays], G)
        out[which] = (img.detach(), dict(zip(B.PARAMS, grads[:4])), grads[4])
        _check(r, E32[name], name + " " + which, img.detach(), out[which][1], groups=B.PARAMS)
    rr = RR.reference(beam + "_p300_small")
    e = RR.load_e32()[beam + "_p300_small"]
    for which in ("bundle", "projector"):
        _bracket(out[which][2].cpu().numpy(), rr["lo"]["grad"], rr["hi"]["grad"], 4.0 * e * rr["hi"]["gabs"] + RR.FLOOR,
                 name + " " + which + " d[V,12]")


# ------------------------------------------------------------------------------------------------------ the C ABI itself
def _guarded(n, dev, dtype=torch.float32):
    """A buffer of n elements with GUARD sentinel elements on either side: (whole, middle view)."""
    whole = torch.full((n + 2 * GUARD,), SENTINEL if dtype == torch.float32 else 0xA5, dtype=dtype, device=dev)
    return whole, whole[GUARD:GUARD + n]


def _guards_intact(whole, n):
    fill = SENTINEL if whole.dtype == torch.float32 else 0xA5
    return bool((whole[:GUARD] == fill).all()) and bool((whole[GUARD + n:] == fill).all())


def _abi(sc, dev, with_rays=True, ws_short=0, stream=None):
    """r2_integrate_gaussians and its backward through ctypes, every output and both workspaces between guard words.
    -> (rc of the forward, rc of the backward, values, grads dict, True when every guard survived, workspace bytes)."""
    from r2_gaussian_amd import _lib
    L = _lib.lib()
    x, d, s, r = _leaves(sc["cloud"], dev)
    rays = torch.cat([torch.from_numpy(sc["origins"]).reshape(-1, 3), torch.from_numpy(sc["directions"]).reshape(-1, 3)], 1).to(dev).contiguous()
    G = torch.from_numpy(sc["G"]).to(dev)
    N, P = rays.shape[0], x.shape[0]
    sizes = {"value": N, "xyz": 3 * P, "density": P, "scaling": 3 * P, "rotation": 4 * P, "rays": 6 * N}
    buf = {k: _guarded(n, dev) for k, n in sizes.items()}
    need = int(L.r2_integrate_gaussians_workspace_bytes(N, P))
    assert need == (24 * (1 + min((P + 255) // 256, 1024) + (N + 255) // 256) if N and P else 0)
    nws = max(need - ws_short, 0)
    ws = [_guarded(nws, dev, torch.uint8) for _ in range(2)]
    st = torch.cuda.current_stream(dev) if stream is None else stream
    st.wait_stream(torch.cuda.current_stream(dev))
    h = st.cuda_stream
    rc1 = L.r2_integrate_gaussians(N, rays.data_ptr(), int(sc["half_line"]), P, x.data_ptr(), d.data_ptr(), s.data_ptr(),
                                   float(sc["mod"]), r.data_ptr(), buf["value"][1].data_ptr(), ws[0][1].data_ptr(), nws, h)
    rc2 = L.r2_integrate_gaussians_backward(N, rays.data_ptr(), int(sc["half_line"]), P, x.data_ptr(), d.data_ptr(), s.data_ptr(),
                                            float(sc["mod"]), r.data_ptr(), G.data_ptr(), buf["xyz"][1].data_ptr(),
                                            buf["density"][1].data_ptr(), buf["scaling"][1].data_ptr(), buf["rotation"][1].data_ptr(),
                                            buf["rays"][1].data_ptr() if with_rays else None, ws[1][1].data_ptr(), nws, h)
    st.synchronize()
    intact = all(_guards_intact(buf[k][0], n) for k, n in sizes.items()) and all(_guards_intact(w[0], nws) for w in ws)
    shapes = {"xyz": (P, 3), "density": (P, 1), "scaling": (P, 3), "rotation": (P, 4)}
    grads = {k: buf[k][1].clone().reshape(shapes[k]) for k in B.PARAMS}
    gr = buf["rays"][1].clone().reshape(N, 6)
    grads["origins"], grads["directions"] = gr[:, :3].reshape(sc["origins"].shape), gr[:, 3:].reshape(sc["origins"].shape)
    return rc1, rc2, buf["value"][1].clone().reshape(sc["origins"].shape[:-1]), grads, intact, need


@pytest.mark.parametrize("name", ["flat_cone", "tail_257", "many"])
def test_guard_words_survive_and_autograd_is_the_c_abi(gpu, name):
    """Guard words around the values, the gradients and both workspaces are untouched, and torch.autograd.grad through
    integrate_rays gives the bits of the C ABI's backward."""
    sc = B.scene(name)
    rc1, rc2, val, grads, intact, _ = _abi(sc, gpu)
    assert rc1 == 0 and rc2 == 0 and intact
    val2, grads2 = _grads(sc, gpu)
    assert torch.equal(val, val2)
    for k in B.GRADS:
        assert torch.equal(grads[k], grads2[k]), k


def test_backward_without_ray_gradients_and_on_another_stream(gpu):
    """dL_drays = NULL: identical parameter gradients, and the ray gradient's buffer is not touched.  A non-default stream
    gives the bits of the default one."""
    sc = B.scene("scattered")
    rc1, rc2, v1, g1, ok1, _ = _abi(sc, gpu)
    rc3, rc4, v2, g2, ok2, _ = _abi(sc, gpu, with_rays=False)
    assert rc1 == rc2 == rc3 == rc4 == 0 and ok1 and ok2
    for k in B.PARAMS:
        assert torch.equal(g1[k], g2[k]), k
    assert (g2["origins"] == SENTINEL).all() and (g2["directions"] == SENTINEL).all()
    rc5, rc6, v3, g3, ok3, _ = _abi(sc, gpu, stream=torch.cuda.Stream(gpu))
    assert rc5 == rc6 == 0 and ok3 and torch.equal(v3, v1)
    for k in B.GRADS:
        assert torch.equal(g3[k], g1[k]), k


def test_short_workspace_is_refused_and_no_rays_are_no_work(gpu):
    from r2_gaussian_amd import _lib
    L = _lib.lib()
    sc = B.scene("tail_257")   # the cloud box, one partial box, two blocks: 96 bytes
    rc1, rc2, val, grads, intact, need = _abi(sc, gpu, ws_short=1)
    assert need == 96 and rc1 == _lib.R2_ERR_INVALID and rc2 == _lib.R2_ERR_INVALID and intact
    msg = L.r2_last_error().decode()
    assert "workspace" in msg and "96" in msg
    assert (val == SENTINEL).all() and all((g == SENTINEL).all() for g in grads.values())   # nothing was launched
    z = torch.zeros(16, device=gpu)
    rc = L.r2_integrate_gaussians(1, z.data_ptr(), 0, 1, z.data_ptr(), z.data_ptr(), z.data_ptr(), 1.0, z.data_ptr(), z.data_ptr(),
                                  None, C.c_size_t(1 << 20), None)
    assert rc == _lib.R2_ERR_INVALID and "workspace" in L.r2_last_error().decode()
    # N = 0: success; the forward touches nothing, the backward writes the zeros of Gaussians no ray touches; no workspace
    empty = dict(sc, origins=sc["origins"][:0], directions=sc["directions"][:0], G=sc["G"][:0])
    rc1, rc2, val, grads, intact, need = _abi(empty, gpu)
    assert need == 0 and rc1 == 0 and rc2 == 0 and intact and val.numel() == 0
    assert all((grads[k] == 0).all() for k in B.PARAMS)


# ------------------------------------------------------------------------------------------------------ the public layer
def test_argument_errors(gpu):
    from r2_gaussian_amd import _lib
    from r2_gaussian_amd.gaussian_projector import integrate_rays
    sc = B.scene("tail_1")
    x, d, s, r = _leaves(sc["cloud"], gpu)
    o, dr = torch.from_numpy(sc["origins"]).to(gpu), torch.from_numpy(sc["directions"]).to(gpu)
    with pytest.raises(_lib.R2HipError):
        integrate_rays(o.cpu(), dr, x, d, s, r)
    with pytest.raises(_lib.R2HipError):
        integrate_rays(o, dr, x.cpu(), d, s, r)
    with pytest.raises(ValueError):
        integrate_rays(o[:, :2], dr[:, :2], x, d, s, r)
    with pytest.raises(ValueError):
        integrate_rays(o, dr.expand(2, 3), x, d, s, r)
    with pytest.raises(ValueError):
        integrate_rays(o, dr, x, d, s[:5], r)
    with pytest.raises(ValueError):
        integrate_rays(o, dr, x, d[:3], s, r)
    assert integrate_rays(o[:0], dr[:0], x, d, s, r).shape == (0,)
    assert integrate_rays(o.expand(4, 5, 3), dr.expand(4, 5, 3), x, d, s, r, sort=True).shape == (4, 5)
