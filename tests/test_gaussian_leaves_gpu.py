"""GPU: the leaf-culled exact line integrals (r2_gaussian_amd.gaussian_projector.integrate_rays(method="leaves");
csrc/gaussian_leaves.hip and its backward) against the float64 restatement of the contract they share with method="blocks"
(tests/gaussian_bundle_ref.py), on that module's scenes and on the scenes at the edges of this kernel
(tests/gaussian_leaves_ref.py).

Tolerance and bracket are tests/test_gaussian_bundle_gpu.py's: 4 x e32 x sum_g |term_g| per ray (and 4 x e32_k x
sum_pairs |contribution| per gradient component), e32 the measured error of the float32 restatement against float64 for that
scene (tests/golden/gaussian_bundle/e32.json, tests/golden/gaussian_leaves/e32.json; the factor 4 is DESIGN.md section 4's for
this family), plus the float32 underflow floor; the kernels must lie between the float64 sum cut at q <= 32 and the float64
sum of every pair, each widened by the tolerance, at every ray and every gradient component.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import gaussian_bundle_ref as B
from tests import gaussian_leaves_ref as LR

pytestmark = pytest.mark.gpu

E32 = dict(B.load_e32(), **LR.load_e32())
GUARD = 16          # guard words on either side of every buffer the C ABI writes
SENTINEL = -7.25


def _reference(name):
    return LR.reference(name) if name in LR.SCENES else B.reference(name)


def _leaves(cloud, dev, grad=False):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(dev).requires_grad_(grad) for a in cloud]


def _integrate(sc, dev, grad=False, **kw):
    """-> (values, [xyz, density, scaling, rotation, origins, directions] leaves)."""
    from r2_gaussian_amd.gaussian_projector import integrate_rays
    leaves = _leaves(sc["cloud"], dev, grad)
    o = torch.from_numpy(sc["origins"]).to(dev).requires_grad_(grad)
    d = torch.from_numpy(sc["directions"]).to(dev).requires_grad_(grad)
    kw.setdefault("method", "leaves")
    return integrate_rays(o, d, *leaves, scale_modifier=sc["mod"], half_line=sc["half_line"], **kw), leaves + [o, d]


def _grads(sc, dev, **kw):
    val, leaves = _integrate(sc, dev, grad=True, **kw)
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


@pytest.mark.parametrize("name", B.SCENES + LR.SCENES)
def test_forward_and_backward_vs_float64(gpu, name):
    """Values and all six gradients (autograd end to end) inside the float64 bracket: on every scene of
    tests/gaussian_bundle_ref.py with that scene's existing e32, and on the scenes of tests/gaussian_leaves_ref.py with their
    own: P = 1, 63, 64, 65, 129 (the leaf tails), 1500 small Gaussians in random index order (24 leaves that all span the
    cloud: nothing culled), the same in cloud_order (most (ray, leaf) pairs culled), with 30 Gaussians 20 x larger, and a
    lattice on which every line meets one sphere."""
    r = _reference(name)
    sc = r["scene"]
    val, grads = _grads(sc, gpu)
    assert val.shape == sc["origins"].shape[:-1] and val.dtype == torch.float32
    _check(r, E32[name], name, val, grads)
    if sc["zero_rays"]:
        zr = sc["zero_rays"]
        assert (val[zr] == 0).all() and (grads["origins"][zr] == 0).all() and (grads["directions"][zr] == 0).all()


def test_one_pair_is_the_blocks_bits(gpu):
    """One term per ray leaves nothing to associate: values and dL_drays are the bits of method="blocks", which pins the
    rule (the pair, the cut, the cone rule, the sphere test) as identical."""
    sc = LR.scene("one_pair")
    v1, g1 = _grads(sc, gpu)
    v2, g2 = _grads(sc, gpu, method="blocks")
    assert (v1 != 0).sum() > 100
    assert torch.equal(v1, v2) and torch.equal(g1["origins"], g2["origins"]) and torch.equal(g1["directions"], g2["directions"])


def _far_rays(n, seed):
    """n rays 50 units and more away: half of them aimed through the cloud, half of them parallel to the x axis at
    |y| >= 40 (they miss every leaf)."""
    g = np.random.RandomState(seed)
    u = g.randn(n, 3)
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    o = 50.0 * u * (1.0 + g.rand(n, 1))
    d = ((g.rand(n, 3) * 2 - 1) * 0.3 - o) * np.exp(g.uniform(-2, 2, (n, 1)))
    o[1::2, 1] = np.where(o[1::2, 1] >= 0, 40.0, -40.0) + o[1::2, 1]
    d[1::2] = (1.0, 0.0, 0.0)
    return o.astype(np.float32), d.astype(np.float32)


@pytest.mark.parametrize("name", ["scattered", "spread_ordered"])
def test_a_ray_does_not_depend_on_the_other_rays(gpu, name):
    """The same rays under a fixed random permutation, with 300 far-away rays interleaved, and with sort=True: values and
    dL_drays per ray are bit-identical; the parameter gradients, whose sums follow the ray order, stay inside the bracket."""
    r = _reference(name)
    sc = r["scene"]
    o, d = sc["origins"].reshape(-1, 3), sc["directions"].reshape(-1, 3)
    v0, g0 = _grads(sc, gpu)
    N = o.shape[0]
    perm = np.random.RandomState(77).permutation(N)
    v1, g1 = _grads(dict(sc, origins=o[perm], directions=d[perm], G=sc["G"][perm]), gpu)
    pt = torch.from_numpy(perm).to(gpu)
    assert torch.equal(v1, v0[pt]) and torch.equal(g1["origins"], g0["origins"][pt]) and torch.equal(g1["directions"], g0["directions"][pt])
    _check(r, E32[name], name + " permuted", None, g1, groups=B.PARAMS)
    fo, fd = _far_rays(300, 78)
    where = np.sort(np.random.RandomState(79).permutation(N + 300)[:N])   # the slots the scene's rays keep, in order
    o2, d2, G2 = np.zeros((N + 300, 3), np.float32), np.zeros((N + 300, 3), np.float32), np.zeros(N + 300, np.float32)
    rest = np.setdiff1d(np.arange(N + 300), where)
    o2[where], d2[where], G2[where], o2[rest], d2[rest] = o, d, sc["G"], fo, fd
    v2, g2 = _grads(dict(sc, origins=o2, directions=d2, G=G2), gpu)
    wt = torch.from_numpy(where).to(gpu)
    assert torch.equal(v2[wt], v0) and torch.equal(g2["origins"][wt], g0["origins"]) and torch.equal(g2["directions"][wt], g0["directions"])
    assert (v2[torch.from_numpy(rest[1::2]).to(gpu)] == 0).all()
    _check(r, E32[name], name + " interleaved", None, g2, groups=B.PARAMS)   # G = 0 on the far rays
    v3, g3 = _grads(sc, gpu, sort=True)
    assert torch.equal(v3, v0) and torch.equal(g3["origins"], g0["origins"]) and torch.equal(g3["directions"], g0["directions"])
    _check(r, E32[name], name + " sorted", None, g3, groups=B.PARAMS)


def test_calls_are_reproducible(gpu):
    sc = LR.scene("spread_ordered")
    v1, g1 = _grads(sc, gpu)
    v2, g2 = _grads(sc, gpu)
    assert torch.equal(v1, v2)
    for k in B.GRADS:
        assert torch.equal(g1[k], g2[k]), k


def test_order(gpu):
    """order=True: values and gradients inside the bracket, the gradients at the caller's indices (the bracket is per
    Gaussian), exact zeros for the Gaussians that contribute nothing; with the cloud already in cloud_order the sort is
    stable, the gathers are copies, and order=True gives the bits of order=False."""
    for name in ("spread", "bad"):
        r = _reference(name)
        val, grads = _grads(r["scene"], gpu, order=True)
        _check(r, E32[name], name + " order=True", val, grads)
    zg = r["scene"]["zero_gaussians"]
    assert len(zg) == 3 and all((grads[k][zg] == 0).all() for k in B.PARAMS)
    sc = LR.scene("mixed")
    v1, g1 = _grads(sc, gpu, order=True)
    v2, g2 = _grads(sc, gpu, order=False)
    assert torch.equal(v1, v2) and (v1 != 0).sum() > 100
    for k in B.GRADS:
        assert torch.equal(g1[k], g2[k]), k


# ------------------------------------------------------------------------------------------------------ the C ABI itself
def _guarded(n, dev, dtype=torch.float32):
    """A buffer of n elements with GUARD sentinel elements on either side: (whole, middle view)."""
    whole = torch.full((n + 2 * GUARD,), SENTINEL if dtype == torch.float32 else 0xA5, dtype=dtype, device=dev)
    return whole, whole[GUARD:GUARD + n]


def _guards_intact(whole, n):
    fill = SENTINEL if whole.dtype == torch.float32 else 0xA5
    return bool((whole[:GUARD] == fill).all()) and bool((whole[GUARD + n:] == fill).all())


def _abi(sc, dev, with_rays=True, ws_short=0, stream=None):
    """r2_integrate_gaussians_leaves and its backward through ctypes, every output and both workspaces between guard words
    (16 bytes of them: the workspace stays aligned).
    -> (rc of the forward, rc of the backward, values, grads dict, True when every guard survived, workspace bytes)."""
    from r2_gaussian_amd import _lib
    L = _lib.lib()
    x, d, s, r = _leaves(sc["cloud"], dev)
    rays = torch.cat([torch.from_numpy(sc["origins"]).reshape(-1, 3), torch.from_numpy(sc["directions"]).reshape(-1, 3)], 1).to(dev).contiguous()
    G = torch.from_numpy(sc["G"]).to(dev)
    N, P = rays.shape[0], x.shape[0]
    sizes = {"value": N, "xyz": 3 * P, "density": P, "scaling": 3 * P, "rotation": 4 * P, "rays": 6 * N}
    buf = {k: _guarded(n, dev) for k, n in sizes.items()}
    need = int(L.r2_integrate_gaussians_leaves_workspace_bytes(N, P))
    assert need == (80 * P + 24 * ((P + 63) // 64) if N and P else 0)
    nws = max(need - ws_short, 0)
    ws = [_guarded(nws, dev, torch.uint8) for _ in range(2)]
    assert all(w[1].data_ptr() % 16 == 0 for w in ws)
    st = torch.cuda.current_stream(dev) if stream is None else stream
    st.wait_stream(torch.cuda.current_stream(dev))
    h = st.cuda_stream
    rc1 = L.r2_integrate_gaussians_leaves(N, rays.data_ptr(), int(sc["half_line"]), P, x.data_ptr(), d.data_ptr(), s.data_ptr(),
                                          float(sc["mod"]), r.data_ptr(), buf["value"][1].data_ptr(), ws[0][1].data_ptr(), nws, h)
    rc2 = L.r2_integrate_gaussians_leaves_backward(N, rays.data_ptr(), int(sc["half_line"]), P, x.data_ptr(), d.data_ptr(),
                                                   s.data_ptr(), float(sc["mod"]), r.data_ptr(), G.data_ptr(), buf["xyz"][1].data_ptr(),
                                                   buf["density"][1].data_ptr(), buf["scaling"][1].data_ptr(),
                                                   buf["rotation"][1].data_ptr(), buf["rays"][1].data_ptr() if with_rays else None,
                                                   ws[1][1].data_ptr(), nws, h)
    st.synchronize()
    intact = all(_guards_intact(buf[k][0], n) for k, n in sizes.items()) and all(_guards_intact(w[0], nws) for w in ws)
    shapes = {"xyz": (P, 3), "density": (P, 1), "scaling": (P, 3), "rotation": (P, 4)}
    grads = {k: buf[k][1].clone().reshape(shapes[k]) for k in B.PARAMS}
    gr = buf["rays"][1].clone().reshape(N, 6)
    grads["origins"], grads["directions"] = gr[:, :3].reshape(sc["origins"].shape), gr[:, 3:].reshape(sc["origins"].shape)
    return rc1, rc2, buf["value"][1].clone().reshape(sc["origins"].shape[:-1]), grads, intact, need


def _scene(name):
    return LR.scene(name) if name in LR.SCENES else B.scene(name)


@pytest.mark.parametrize("name", ["tail_257", "many", "spread"])
def test_guard_words_survive_and_autograd_is_the_c_abi(gpu, name):
    """Guard words around the values, the gradients and both workspaces are untouched, and torch.autograd.grad through
    integrate_rays(method="leaves") gives the bits of the C ABI's backward."""
    sc = _scene(name)
    rc1, rc2, val, grads, intact, _ = _abi(sc, gpu)
    assert rc1 == 0 and rc2 == 0 and intact
    val2, grads2 = _grads(sc, gpu)
    assert torch.equal(val, val2) and (val != 0).sum() > 20
    for k in B.GRADS:
        assert torch.equal(grads[k], grads2[k]), k


def test_backward_without_ray_gradients_and_on_another_stream(gpu):
    """dL_drays = NULL: identical parameter gradients, and the ray gradient's buffer is not touched.  A non-default stream
    gives the bits of the default one."""
    sc = LR.scene("spread")
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


def test_short_workspace_is_refused_and_no_rays_and_no_cloud(gpu):
    from r2_gaussian_amd import _lib
    L = _lib.lib()
    sc = B.scene("tail_257")   # 40 Gaussians: 3200 bytes and one leaf box
    rc1, rc2, val, grads, intact, need = _abi(sc, gpu, ws_short=1)
    assert need == 3224 and rc1 == _lib.R2_ERR_INVALID and rc2 == _lib.R2_ERR_INVALID and intact
    msg = L.r2_last_error().decode()
    assert "workspace" in msg and "3224" in msg
    assert (val == SENTINEL).all() and all((g == SENTINEL).all() for g in grads.values())   # nothing was launched
    z = torch.zeros(16, device=gpu)
    rc = L.r2_integrate_gaussians_leaves(1, z.data_ptr(), 0, 1, z.data_ptr(), z.data_ptr(), z.data_ptr(), 1.0, z.data_ptr(),
                                         z.data_ptr(), None, C.c_size_t(1 << 20), None)
    assert rc == _lib.R2_ERR_INVALID and "workspace" in L.r2_last_error().decode()
    # N = 0: success; the forward touches nothing, the backward writes the zeros of Gaussians no ray touches; no workspace
    empty = dict(sc, origins=sc["origins"][:0], directions=sc["directions"][:0], G=sc["G"][:0])
    rc1, rc2, val, grads, intact, need = _abi(empty, gpu)
    assert need == 0 and rc1 == 0 and rc2 == 0 and intact and val.numel() == 0
    assert all((grads[k] == 0).all() for k in B.PARAMS)
    # P = 0: zeros for the values and the ray gradients; no workspace
    rc1, rc2, val, grads, intact, need = _abi(B.scene("none"), gpu)
    assert need == 0 and rc1 == 0 and rc2 == 0 and intact
    assert (val == 0).all() and (grads["origins"] == 0).all() and (grads["directions"] == 0).all()


# ------------------------------------------------------------------------------------------------------ the public layer
def test_argument_errors(gpu):
    from r2_gaussian_amd.gaussian_projector import integrate_rays
    from r2_gaussian_amd.geometry import refine_geometry
    sc = B.scene("tail_1")
    x, d, s, r = _leaves(sc["cloud"], gpu)
    o, dr = torch.from_numpy(sc["origins"]).to(gpu), torch.from_numpy(sc["directions"]).to(gpu)
    with pytest.raises(ValueError):
        integrate_rays(o, dr, x, d, s, r, method="tree")
    with pytest.raises(ValueError):
        integrate_rays(o, dr, x, d, s, r, method="blocks", order=True)
    with pytest.raises(ValueError):
        integrate_rays(o, dr, x, d, s, r, order=True)
    assert integrate_rays(o[:0], dr[:0], x, d, s, r, method="leaves").shape == (0,)
    assert integrate_rays(o.expand(4, 5, 3), dr.expand(4, 5, 3), x, d, s, r, sort=True, method="leaves", order=True).shape == (4, 5)
    rays = torch.zeros(3, 12, device=gpu)
    for bad in (0, -1, 3 * 17 * 23 + 1):
        with pytest.raises(ValueError):
            refine_geometry(torch.zeros(3, 17, 23, device=gpu), (x, d, s, r), lambda p: rays, {"offDetector": torch.zeros(2, device=gpu)}, 1, 0.1,
                            rays_per_step=bad)


def _refine(gpu, **kw):
    from r2_gaussian_amd.geometry import refine_geometry
    from tests import gaussian_project_rays_ref as Q
    gold, st = Q.load_refine(), Q.refine_setup()
    projs = torch.from_numpy(st["projs"]).to(gpu)
    start = {"offDetector": torch.zeros(2, dtype=torch.float64, device=gpu)}
    got, hist = refine_geometry(projs, _leaves(st["cloud"], gpu), Q.refine_rays_fn(st, gpu), start, gold["K"], gold["lr"], **kw)
    assert (start["offDetector"] == 0).all() and hist.shape == (gold["K"],) and hist.is_cuda
    return gold, st, got["offDetector"].cpu().numpy(), hist


def test_refinement_with_every_pixel_follows_the_host_loop(gpu):
    """refine_geometry(rays_per_step=V*H*W): every pixel appears once per step, so the loss is the full loss up to the
    association of its sum, and the final offDetector must meet the bound of the refinement over whole views
    (tests/test_gaussian_project_rays_gpu.py): within 4 x max |float32 loop - float64 loop| of the float64 loop's."""
    gold, st, p, hist = _refine(gpu, rays_per_step=3 * 17 * 23)
    dist, tol = float(np.abs(p - np.asarray(gold["final64"])).max()), 4.0 * gold["f32_minus_f64"]
    print("refinement, every pixel: offDetector %s, float64 loop %s, distance %.3e, tolerance %.3e; loss %.3e -> %.3e"
          % (p, gold["final64"], dist, tol, float(hist[0]), float(hist[-1])))
    assert dist <= tol


def test_refinement_with_a_quarter_of_the_pixels_converges(gpu):
    """refine_geometry(rays_per_step=REFINE_RAYS, seed=REFINE_SEED): the final offset error is below half the initial one,
    as the CPU tests check for the same loop on the host in float64."""
    gold, st, p, hist = _refine(gpu, rays_per_step=LR.REFINE_RAYS, seed=LR.REFINE_SEED)
    err = float(np.abs(p - np.asarray(gold["true_offDetector"])).max())
    print("refinement, %d pixels per step: offDetector %s, error %.3e of initially %.3e; loss %.3e -> %.3e"
          % (LR.REFINE_RAYS, p, err, gold["initial_error64"], float(hist[0]), float(hist[-1])))
    assert err < 0.5 * gold["initial_error64"]
