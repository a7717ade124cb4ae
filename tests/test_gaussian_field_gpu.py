"""GPU: the exact field query (r2_gaussian_amd.field; csrc/gaussian_query.hip and its backward) against the float64
restatement of its contract (tests/gaussian_field_ref.py).

Tolerance: 4 x e32 x sum_g |term_g| per point (and 4 x e32_k x sum_pairs |contribution| per gradient component), e32 being the
measured error of the float32 restatement against float64 for that scene (tests/golden/gaussian_field/e32.json; the factor 4
is DESIGN.md section 4's: the device's expf / division against numpy's and the different association of the sums), plus the
float32 underflow floor of the reference module.  Bracket: the contract lets a pair with q > 32 be summed or skipped, so the
kernels must lie between the float64 sum cut at q <= 32 and the float64 sum of every pair, each widened by the tolerance, at
every point and every gradient component; none is excluded.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import gaussian_field_ref as R

pytestmark = pytest.mark.gpu

E32 = R.load_e32()
GUARD = 16          # guard words on either side of every buffer the C ABI writes
SENTINEL = -7.25


def _leaves(cloud, dev, grad=False):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(dev).requires_grad_(grad) for a in cloud]


def _query(sc, dev, grad=False, sort=False):
    """-> (values, [xyz, density, scaling, rotation, points] leaves)."""
    from r2_gaussian_amd.field import query_points
    leaves = _leaves(sc["cloud"], dev, grad)
    pts = torch.from_numpy(sc["points"]).to(dev).requires_grad_(grad)
    return query_points(pts, *leaves, scale_modifier=sc["mod"], sort=sort), leaves + [pts]


def _grads(sc, dev, sort=False):
    val, leaves = _query(sc, dev, grad=True, sort=sort)
    G = torch.from_numpy(sc["G"]).to(dev).reshape(val.shape)
    return val.detach(), dict(zip(R.GRADS, torch.autograd.grad(val, leaves, G)))


def _bracket(got, a, b, tol, what):
    got = np.asarray(got, np.float64).reshape(a.shape)
    lo, hi = np.minimum(a, b) - tol, np.maximum(a, b) + tol
    bad = (got < lo) | (got > hi) | ~np.isfinite(got)
    worst = float(np.max(np.maximum(lo - got, got - hi) / np.maximum(tol, 1e-300))) if got.size else -1.0
    print("%s: worst excess over the bracket in units of the tolerance %.3f (1 + this <= 1 passes)" % (what, worst))
    assert not bad.any(), "%s: %d of %d outside the bracket, worst excess %.3g tolerances" % (what, int(bad.sum()), bad.size, worst)


def _check(name, val, grads, factor=4.0):
    r = R.reference(name)
    _bracket(val.cpu().numpy(), r["lo"]["val"], r["hi"]["val"], factor * E32[name]["value"] * r["hi"]["abs"] + R.FLOOR, name + " value")
    for k in R.GRADS:
        tol = factor * E32[name][k] * r["hi"]["gabs"][k] + R.FLOOR
        _bracket(grads[k].cpu().numpy(), r["lo"]["grads"][k], r["hi"]["grads"][k], tol, name + " d" + k)


@pytest.mark.parametrize("name", R.SCENES)
def test_forward_and_backward_vs_float64(gpu, name):
    """Values and all five gradients (autograd end to end) inside the float64 bracket on every scene of the reference
    module: an oblique plane, a 12^3 patch, scattered points, the block tails N = 1, 255, 256, 257, 513, P = 700 (two full
    rounds of 256 and a partial one), P = 0, points outside every sphere, cloud and points 100 extents away, sigma = 5e-4,
    non-finite rows and points, raw quaternions of norm 0.3 .. 3, scale_modifier 0.5 and 2."""
    sc = R.reference(name)["scene"]
    val, grads = _grads(sc, gpu)
    assert val.shape == sc["points"].shape[:-1] and val.dtype == torch.float32
    _check(name, val, grads)


@pytest.mark.parametrize("name", ["far", "none", "bad"])
def test_exact_zeros(gpu, name):
    """Points outside every sphere and P = 0: zeros everywhere.  `bad`: exact zeros for the gradients of the Gaussians with a
    NaN mean, an inf scale, a zero scale, and for the value and gradient of the NaN and inf points; everything finite; the
    values of the good points are bit-identical to the query without the bad Gaussians."""
    sc = R.reference(name)["scene"]
    val, grads = _grads(sc, gpu)
    if name in ("far", "none"):
        assert (val == 0).all()
        assert all((g == 0).all() for g in grads.values())
        return
    zg, zp = sc["zero_gaussians"], sc["zero_points"]
    assert torch.isfinite(val).all() and all(torch.isfinite(g).all() for g in grads.values())
    assert (val[zp] == 0).all() and (grads["points"][zp] == 0).all()
    for k in R.GRADS[:4]:
        assert (grads[k][zg] == 0).all()
    keep = [i for i in range(sc["cloud"][0].shape[0]) if i not in zg]
    val2, _ = _query(dict(sc, cloud=tuple(a[keep] for a in sc["cloud"])), gpu)
    assert torch.equal(val, val2)


def test_calls_are_reproducible(gpu):
    sc = R.scene("plane")
    v1, g1 = _grads(sc, gpu)
    v2, g2 = _grads(sc, gpu)
    assert torch.equal(v1, v2)
    for k in R.GRADS:
        assert torch.equal(g1[k], g2[k]), k


# ------------------------------------------------------------------------------------------------------ the C ABI itself
def _guarded(n, dev, dtype=torch.float32):
    """A buffer of n elements with GUARD sentinel elements on either side: (whole, middle view)."""
    whole = torch.full((n + 2 * GUARD,), SENTINEL if dtype == torch.float32 else 0xA5, dtype=dtype, device=dev)
    return whole, whole[GUARD:GUARD + n]


def _guards_intact(whole, n):
    fill = SENTINEL if whole.dtype == torch.float32 else 0xA5
    return bool((whole[:GUARD] == fill).all()) and bool((whole[GUARD + n:] == fill).all())


def _abi(sc, dev, with_points=True, ws_bytes=None):
    """r2_query_gaussians and its backward through ctypes, every output and the workspace between guard words.
    -> (rc of the backward, values, grads dict, True when every guard survived)."""
    from r2_gaussian_amd import _lib
    L = _lib.lib()
    x, d, s, r = _leaves(sc["cloud"], dev)
    pts = torch.from_numpy(sc["points"]).to(dev).reshape(-1, 3).contiguous()
    G = torch.from_numpy(sc["G"]).to(dev)
    N, P = pts.shape[0], x.shape[0]
    sizes = {"value": N, "xyz": 3 * P, "density": P, "scaling": 3 * P, "rotation": 4 * P, "points": 3 * N}
    buf = {k: _guarded(n, dev) for k, n in sizes.items()}
    need = int(L.r2_query_gaussians_workspace_bytes(N))
    assert need == 24 * ((N + 255) // 256)
    nws = need if ws_bytes is None else ws_bytes
    ws = _guarded(nws, dev, torch.uint8)
    stream = torch.cuda.current_stream(dev).cuda_stream
    rc = L.r2_query_gaussians(N, pts.data_ptr(), P, x.data_ptr(), d.data_ptr(), s.data_ptr(), float(sc["mod"]), r.data_ptr(),
                              buf["value"][1].data_ptr(), stream)
    assert rc == 0
    rc = L.r2_query_gaussians_backward(N, pts.data_ptr(), P, x.data_ptr(), d.data_ptr(), s.data_ptr(), float(sc["mod"]),
                                       r.data_ptr(), G.data_ptr(), buf["xyz"][1].data_ptr(), buf["density"][1].data_ptr(),
                                       buf["scaling"][1].data_ptr(), buf["rotation"][1].data_ptr(),
                                       buf["points"][1].data_ptr() if with_points else None, ws[1].data_ptr(), nws, stream)
    torch.cuda.synchronize(dev)
    intact = all(_guards_intact(buf[k][0], n) for k, n in sizes.items()) and _guards_intact(ws[0], nws)
    shapes = {"xyz": (P, 3), "density": (P, 1), "scaling": (P, 3), "rotation": (P, 4), "points": sc["points"].shape}
    grads = {k: buf[k][1].clone().reshape(shapes[k]) for k in R.GRADS}
    return rc, buf["value"][1].clone().reshape(sc["points"].shape[:-1]), grads, intact


@pytest.mark.parametrize("name", ["plane", "tail_257", "many"])
def test_guard_words_survive_and_autograd_is_the_c_abi(gpu, name):
    """Guard words around the values, the five gradients and the workspace are untouched, and torch.autograd.grad through
    query_points gives the bits of the C ABI's backward."""
    sc = R.scene(name)
    rc, val, grads, intact = _abi(sc, gpu)
    assert rc == 0 and intact
    val2, grads2 = _grads(sc, gpu)
    assert torch.equal(val, val2)
    for k in R.GRADS:
        assert torch.equal(grads[k], grads2[k]), k


def test_backward_without_point_gradients(gpu):
    """dL_dpoints = NULL: identical parameter gradients, and the point gradient's buffer is not touched."""
    sc = R.scene("scattered")
    rc1, _, g1, ok1 = _abi(sc, gpu)
    rc2, _, g2, ok2 = _abi(sc, gpu, with_points=False)
    assert rc1 == 0 and rc2 == 0 and ok1 and ok2
    for k in R.GRADS[:4]:
        assert torch.equal(g1[k], g2[k]), k
    assert (g2["points"] == SENTINEL).all()


def test_short_workspace_is_refused(gpu):
    from r2_gaussian_amd import _lib
    sc = R.scene("tail_257")   # two blocks: 48 bytes
    rc, _, grads, intact = _abi(sc, gpu, ws_bytes=47)
    assert rc == _lib.R2_ERR_INVALID and intact
    msg = _lib.lib().r2_last_error().decode()
    assert "workspace" in msg and "48" in msg
    assert all((g == SENTINEL).all() for g in grads.values())   # nothing was launched
    L = _lib.lib()
    z = torch.zeros(16, device=gpu)
    rc = L.r2_query_gaussians_backward(1, z.data_ptr(), 1, z.data_ptr(), z.data_ptr(), z.data_ptr(), 1.0, z.data_ptr(), z.data_ptr(),
                                       z.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr(), None, None, C.c_size_t(1 << 20), None)
    assert rc == _lib.R2_ERR_INVALID and "workspace" in L.r2_last_error().decode()


# ------------------------------------------------------------------------------------------------------ the public layer
@pytest.mark.parametrize("name", ["scattered", "far"])
def test_sorted_query_equals_the_unsorted(gpu, name):
    """sort=True against sort=False: within twice the tolerance (each is within one of float64; the parameter sums associate
    differently), inside the bracket itself, and bit for bit where no pair has q > 32 to disagree about."""
    sc = R.reference(name)["scene"]
    v0, g0 = _grads(sc, gpu)
    v1, g1 = _grads(sc, gpu, sort=True)
    _check(name, v1, g1)
    if name == "far":
        assert torch.equal(v0, v1) and all(torch.equal(g0[k], g1[k]) for k in R.GRADS)
        return
    r = R.reference(name)["hi"]
    assert (np.abs((v0 - v1).cpu().numpy().astype(np.float64)) <= 8.0 * E32[name]["value"] * r["abs"] + R.FLOOR).all()
    for k in R.GRADS:
        diff = np.abs((g0[k] - g1[k]).cpu().numpy().astype(np.float64)).reshape(r["gabs"][k].shape)
        assert (diff <= 8.0 * E32[name][k] * r["gabs"][k] + R.FLOOR).all(), k


def test_query_plane_is_query_points_on_the_lattice(gpu):
    from r2_gaussian_amd.field import plane_points, query_plane, query_points
    sc = R.scene("plane")
    leaves = _leaves(sc["cloud"], gpu)
    img = query_plane(R.PLANE["origin"], R.PLANE["du"], R.PLANE["dv"], R.PLANE["H"], R.PLANE["W"], *leaves)
    pts = plane_points(device=gpu, **R.PLANE)
    assert img.shape == (R.PLANE["H"], R.PLANE["W"]) and pts.shape == (R.PLANE["H"], R.PLANE["W"], 3)
    assert torch.equal(img, query_points(pts, *leaves))
    assert np.abs(pts.cpu().numpy() - sc["points"]).max() <= 1e-6   # the lattice the reference scene uses


def test_voxelizer_volume_lies_in_the_field_bracket(gpu):
    """The HIP voxelizer's volume of the 16^3 scene of 150 Gaussians inside the bracket the CPU test holds the oracle's to
    (tests/gaussian_field_ref.voxel_bracket), and the exact query at the voxel centres inside [hi's lower edge, hi]."""
    from r2_gaussian_amd import GaussianVoxelizationSettings, GaussianVoxelizer
    from r2_gaussian_amd.field import query_points, voxel_centres
    b = R.voxel_bracket()
    leaves = _leaves(b["cloud"], gpu)
    n, s, c = b["nVoxel"], b["sVoxel"], b["center"]
    vs = GaussianVoxelizationSettings(1.0, n[0], n[1], n[2], s[0], s[1], s[2], c[0], c[1], c[2], False, False)
    vol, _ = GaussianVoxelizer(vs)(leaves[0], leaves[1], scales=leaves[2], rotations=leaves[3])
    vol = vol.cpu().numpy().astype(np.float64)
    print("voxelizer: min (vol - lo) %.3e, min (hi - vol) %.3e" % ((vol - b["lo"]).min(), (b["hi"] - vol).min()))
    assert (vol >= b["lo"]).all() and (vol <= b["hi"]).all()
    exact = query_points(voxel_centres(c, n, s, gpu), *leaves).cpu().numpy().astype(np.float64)
    assert exact.shape == vol.shape and (exact >= b["lo"]).all() and (exact <= b["hi"]).all()


def test_evaluate_volume_exact_field(gpu):
    """exact_field=True adds vol_exact, psnr_3d_exact and ssim_3d_exact; off, the dictionary has the keys it had before and
    the same values."""
    from r2_gaussian_amd import model_io
    g = np.random.RandomState(2)
    P = 60
    model = {"xyz": torch.tensor((g.rand(P, 3) - 0.5) * 1.2, dtype=torch.float32, device=gpu),
             "density": torch.tensor(g.randn(P, 1) - 1.0, dtype=torch.float32, device=gpu),
             "scaling": torch.tensor(g.randn(P, 3), dtype=torch.float32, device=gpu),
             "rotation": torch.tensor(g.randn(P, 4), dtype=torch.float32, device=gpu), "scale_bound": (0.05, 0.3)}
    cfg = {"nVoxel": (16, 12, 20), "sVoxel": (2.0, 1.5, 2.5), "offOrigin": (0.1, 0.0, -0.1)}
    off = model_io.evaluate_volume(model, cfg)
    gt = off["vol"].clone() * 0.9 + 0.01
    off = model_io.evaluate_volume(model, cfg, vol_gt=gt)
    on = model_io.evaluate_volume(model, cfg, vol_gt=gt, exact_field=True)
    assert sorted(off) == ["psnr_3d", "radii", "ssim_3d", "ssim_3d_x", "ssim_3d_y", "ssim_3d_z", "vol"]
    assert sorted(set(on) - set(off)) == ["psnr_3d_exact", "ssim_3d_exact", "vol_exact"]
    assert torch.equal(on["vol"], off["vol"])
    assert len(on["radii"]) == len(off["radii"]) == 3 and all(torch.equal(a, b) for a, b in zip(on["radii"], off["radii"]))
    assert all(on[k] == off[k] for k in off if k not in ("vol", "radii"))
    assert on["vol_exact"].shape == on["vol"].shape
    # the voxelizer only cuts: the exact field is nowhere below it (beyond rounding) and close to it
    assert (on["vol_exact"] >= on["vol"] - 1e-4 * on["vol"].abs().max()).all()
    assert on["psnr_3d_exact"] == model_io.metric_vol(gt, on["vol_exact"], "psnr")[0]
    assert on["ssim_3d_exact"] == model_io.metric_vol(gt.cpu(), on["vol_exact"].cpu(), "ssim")[0]
    # the device metrics against the host's, at the tolerances tests/test_metrics_gpu.py holds them to
    dev = model_io.evaluate_volume(model, cfg, vol_gt=gt, metrics="device", exact_field=True)
    assert torch.equal(dev["vol_exact"], on["vol_exact"])
    assert abs(dev["psnr_3d_exact"] - on["psnr_3d_exact"]) <= 1e-4 and abs(dev["ssim_3d_exact"] - on["ssim_3d_exact"]) <= 1e-5


def test_argument_errors(gpu):
    from r2_gaussian_amd import _lib
    from r2_gaussian_amd.field import query_plane, query_points, voxel_centres
    sc = R.scene("tail_1")
    x, d, s, r = _leaves(sc["cloud"], gpu)
    pts = torch.from_numpy(sc["points"]).to(gpu)
    with pytest.raises(_lib.R2HipError):
        query_points(pts.cpu(), x, d, s, r)
    with pytest.raises(_lib.R2HipError):
        query_points(pts, x.cpu(), d, s, r)
    with pytest.raises(_lib.R2HipError):
        query_plane((0, 0, 0), (1, 0, 0), (0, 1, 0), 2, 2, x.cpu(), d, s, r)
    with pytest.raises(ValueError):
        query_points(pts[:, :2], x, d, s, r)
    with pytest.raises(ValueError):
        query_points(pts, x, d, s[:5], r)
    with pytest.raises(ValueError):
        query_points(pts, x, d, s, r[:, :3])
    with pytest.raises(ValueError):
        query_points(pts, x, d[:3], s, r)
    with pytest.raises(ValueError):
        query_plane((0, 0, 0), (1, 0, 0), (0, 1, 0), 0, 2, x, d, s, r)
    with pytest.raises(ValueError):
        voxel_centres((0, 0, 0), (4, 0, 4), (1, 1, 1))
    assert query_points(pts[:0], x, d, s, r).shape == (0,)
