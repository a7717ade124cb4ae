"""CPU: the restatement of the volume renderer (tests/volume_render_ref.py) against closed forms and against its own
conservative brick test by brute force; the stored e32; volume_render.py's host side -- transfer functions, cameras, the PNG
writer, the driver's defaults -- and its refusals, which come before the library is touched."""
import math
import struct
import zlib

import numpy as np
import pytest
import torch

from r2_gaussian_amd import _lib
from r2_gaussian_amd import projector as PJ
from r2_gaussian_amd import scene as S
from r2_gaussian_amd import volume_render as VR
from r2_gaussian_amd._lib import R2HipError
from tests import projector_ref as PR
from tests import volume_render_ref as R

U = 2.0 ** -24


# ---- the stored error ------------------------------------------------------------------------------------------------------------

def test_stored_e32_matches_a_fresh_measurement():
    """tests/golden/volume_render/e32.json (python -m tests.volume_render_ref) within 10 % of a fresh measurement."""
    stored = R.load_e32()
    assert set(stored) == set(R.CASES)
    for name in R.CASES:
        fresh = R.measure_e32(name)
        print("%s: stored %.3e, fresh %.3e (%.1f u)" % (name, stored[name], fresh, fresh / U))
        assert abs(fresh - stored[name]) <= 0.1 * stored[name]


# ---- closed forms ------------------------------------------------------------------------------------------------------------------

def _axis_ray(n, axis, dv):
    """One parallel ray along `axis` through the middle of the volume (off the integer planes)."""
    a = np.zeros(3)
    a[axis] = 1.0
    p = np.array([(m - 1) / 2 + 0.25 for m in n])
    p[axis] = -5.0
    return np.concatenate([a, p, [0, 0, 0], [0, 0, 0]])[None].astype(np.float32)


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_constant_extinction_absorbs_over_the_whole_support(axis):
    """A value-independent table of extinction sigma: alpha = 1 - exp(-sigma (n + 1) dVoxel) on an axis-parallel ray through
    the middle -- the support of the interpolant is [-1, n]."""
    n, dv, sigma = (6, 9, 4), (0.11, 0.07, 0.13), 1.7
    vol = np.full(n, 0.4, np.float32)
    w = R.walk(vol, _axis_ray(n, axis, dv), False, 1, 1, dv, 0.5)
    lut = np.array([[1, 1, 1, sigma], [1, 1, 1, sigma]], np.float32)
    want = 1.0 - math.exp(-float(np.float32(sigma)) * (n[axis] + 1) * dv[axis])
    for dtype, tol in ((np.float64, 4 * U), (np.float32, 64 * U)):
        out, used = R.composite(w, lut, 0.0, 1.0, dtype=dtype)
        assert used[0] == w["n"][0] == math.ceil((n[axis] + 1) / 0.5)
        print("axis %d %s: alpha %.9f, closed form %.9f" % (axis, dtype.__name__, out[0, 3], want))
        assert abs(out[0, 3] - want) <= tol
        assert np.allclose(out[0, :3], out[0, 3], rtol=0, atol=tol)   # colour 1: C = 1 - T


def test_beer_lambert_against_the_projector_restatement():
    """A table whose extinction is linear in the value, colour 1: alpha = 1 - exp(-kappa * line integral), the line integral
    being tests/projector_ref.project's on the same rays."""
    c = R.case("inside_cone")
    kappa, hi = 2.5, 1.0
    lut = np.array([[1, 1, 1, 0.0], [1, 1, 1, kappa * hi]], np.float32)
    w = c["walk"]
    ref = PR.project(c["vol"], c["rays"], c["cone"], c["dVoxel"], c["accuracy"], c["H"], c["W"])
    same = (ref["n"] == w["n"]) & ~ref["hitmiss"]            # pixels whose float32 sample count is the float64 one
    assert same.mean() > 0.9
    want = 1.0 - np.exp(-kappa * ref["value"])
    out64, _ = R.composite(w, lut, 0.0, hi, dtype=np.float64)
    out32, _ = R.composite(w, lut, 0.0, hi, dtype=np.float32)
    tol = kappa * ref["bound"] + 8 * U
    err64, err32 = np.abs(out64[:, 3] - want)[same], np.abs(out32[:, 3] - want)[same]
    print("Beer-Lambert: worst f64 %.3e, f32 %.3e, tolerance from %.3e" % (err64.max(), err32.max(), tol[same].min()))
    assert (err64 <= tol[same]).all()
    assert (err32 <= tol[same] + 4 * R.measure_e32("inside_cone") + 64 * U).all()
    assert (out64[~w["hit"]] == 0).all()


def test_nan_lands_on_row_zero_and_early_termination_stops():
    x, i = R._cell(np.array([np.nan, -np.inf, np.inf, 0.5], np.float32), np.float32(0), np.float32(255), 256)
    assert x.tolist() == [0.0, 0.0, 255.0, 127.5] and i.tolist() == [0, 0, 254, 127]
    c = R.case("dense_orbit")
    full, used_full = R.composite(c["walk"], c["lut"], *c["clim"])
    cut, used = R.composite(c["walk"], c["lut"], *c["clim"], t_stop=0.25)
    assert (used <= used_full).all() and (used < used_full).any()
    assert np.abs(full - cut).max() <= 0.25 + 64 * U            # what is left behind a stopped ray is at most T


# ---- the brick test, by brute force ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(R.CASES))
def test_no_sample_leaves_its_bricks_range_and_no_skipped_sample_absorbs(name):
    c = R.case(name)
    w, lut = c["walk"], c["lut"]
    table = R.bricks(c["vol"])
    lo, hi = (a.ravel() for a in R.brick_range(table))
    on = w["brick"] >= 0
    b, f = w["brick"][on], w["f"][on]
    assert on.sum() == w["n"].sum() and b.max() < lo.size
    assert (f >= lo[b]).all() and (f <= hi[b]).all()            # the MIP test and the premise of the compositing test
    empty = R.empty_bricks(table, lut, *c["clim"]).ravel()
    K = len(lut)
    x, i = R._cell(f, np.float32(c["clim"][0]), np.float32(K - 1) / (np.float32(c["clim"][1]) - np.float32(c["clim"][0])), K)
    ext = lut[i, 3] + (x - i.astype(np.float32)) * (lut[i + 1, 3] - lut[i, 3])
    skipped = empty[b]
    print("%s: %d of %d bricks empty, %d of %d samples in them" % (name, empty.sum(), empty.size, skipped.sum(), skipped.size))
    assert (ext[skipped] == 0).all()


def test_the_sparse_case_is_mostly_empty():
    c = R.case("sparse_blobs")
    empty = R.empty_bricks(R.bricks(c["vol"]), c["lut"], *c["clim"])
    assert empty.size == 64 and empty.mean() >= 0.5
    assert (empty.ravel()[c["walk"]["brick"][c["walk"]["brick"] >= 0]]).mean() >= 0.5   # and the rays do cross them


def test_bricks_of_a_hand_made_volume():
    vol = np.zeros((17, 8, 9), np.float32)
    vol[8, 3, 8] = 2.0        # voxel 8 is the ninth of brick 0 and the first of brick 1
    vol[16, 0, 0] = -3.0
    t = R.bricks(vol)
    assert t.shape == (3, 1, 2, 2)
    assert t[0, 0, 0].tolist() == [0.0, 2.0] and t[1, 0, 0].tolist() == [-3.0, 2.0] and t[1, 0, 1].tolist() == [0.0, 2.0]
    assert t[2, 0, 0].tolist() == [-3.0, 0.0] and t[2, 0, 1].tolist() == [0.0, 0.0]


# ---- transfer functions ------------------------------------------------------------------------------------------------------------

def test_transfer_function_edges():
    t = VR.transfer_function("gray", "linear", unit=0.25, K=2)
    assert t.dtype == np.float32 and t.shape == (2, 4)
    assert t[0].tolist() == [0.0, 0.0, 0.0, 0.0]                                    # a = 0: no extinction at all
    assert t[1, :3].tolist() == [1.0, 1.0, 1.0] and t[1, 3] == np.float32(24 * math.log(2) / 0.25)   # a = 1: finite
    assert np.array_equal(VR.transfer_function("gray", "linear", unit=0.3), R.ramp_lut(256, 0.3))
    t = VR.transfer_function("viridis", 0.5, unit=2.0, K=7)
    assert np.allclose(t[:, 3], math.log(2) / 2.0) and t.shape == (7, 4)
    t = VR.transfer_function(np.array([[0, 0, 0], [1, 0.5, 0]]), [0.0, 0.2, 0.0], unit=1.0, K=5)
    assert np.allclose(t[:, 1], [0, 0.125, 0.25, 0.375, 0.5]) and np.allclose(t[:, 3], -np.log1p(-np.array([0, 0.1, 0.2, 0.1, 0])))
    t = VR.transfer_function(np.array([[0, 0, 0, 0.0], [1, 1, 1, 0.5]]), None, unit=1.0, K=3)
    assert np.allclose(t[:, 3], -np.log1p(-np.array([0, 0.25, 0.5])))
    assert np.array_equal(VR.transfer_function("viridis", np.linspace(0, 1, 256), unit=1.0),
                          VR.transfer_function("viridis", "linear", unit=1.0))
    for kw in (dict(K=1), dict(K=1025), dict(unit=None), dict(unit=0.0), dict(opacity=1.5), dict(opacity="sigmoid"),
               dict(opacity=None), dict(opacity=[0.1]), dict(cmap=np.zeros((4, 2))), dict(cmap="no such colormap")):
        with pytest.raises(ValueError):
            VR.transfer_function(**dict(dict(unit=1.0), **kw))


def test_committed_viridis_is_matplotlibs():
    matplotlib = pytest.importorskip("matplotlib")
    from r2_gaussian_amd._viridis import VIRIDIS
    assert np.array_equal(np.asarray(VIRIDIS), np.asarray(matplotlib.colormaps["viridis"](np.arange(256)))[:, :3])
    assert np.array_equal(VR.transfer_function("viridis", "linear", unit=1.0)[:, :3], np.asarray(VIRIDIS, np.float32))
    plasma = VR.transfer_function("plasma", "linear", unit=1.0, K=16)
    assert np.allclose(plasma[:, :3], np.asarray(matplotlib.colormaps["plasma"](np.linspace(0, 1, 16)))[:, :3])


# ---- cameras -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["cone", "parallel"])
def test_look_at_rays_is_ray_params_of_the_same_pose(mode):
    """A scene.make_view camera and a look_at_rays camera at its pose give the same twelve numbers, up to the float32
    rounding of the view's matrices (ray_params reads them; look_at_rays derives everything in float64)."""
    cfg = dict(S.CONE_BEAM if mode == "cone" else S.PARALLEL_BEAM, nVoxel=[16, 20, 24])
    n, sV, ctr, H = cfg["nVoxel"], cfg["sVoxel"], cfg["offOrigin"], 12
    for angle in (0.0, 0.7, 2.9, 4.4):
        view = S.make_view(angle, (H, H), cfg)
        want = PJ.ray_params([view], sV, ctr, n)
        eye = np.array([cfg["DSO"] * math.cos(angle), cfg["DSO"] * math.sin(angle), 0.0])
        kw = (dict(fov_y=math.degrees(2 * math.atan2(cfg["sDetector"][0] / 2, cfg["DSD"]))) if mode == "cone"
              else dict(ortho_height=2.0))
        got, cone = VR.look_at_rays(eye, ctr, (0, 0, 1), H, H, sV, ctr, n, **kw)
        assert cone == (mode == "cone") and got.shape == (1, 12) and got.dtype == np.float32
        # a float32 matrix entry is off by u relative; a position of magnitude |eye| + 1 maps to index units by 1 / dVoxel
        tol = 16 * U * (cfg["DSO"] + 1) * max(m / s for m, s in zip(n, sV))
        print("%s angle %.1f: worst difference %.3e, tolerance %.3e" % (mode, angle, np.abs(got - want).max(), tol))
        assert np.abs(got - want).max() <= tol
    assert np.array_equal(VR.view_rays([view], sV, ctr, n), want)
    # the test's own camera restates it too
    mine, _ = R.camera_rays(eye, (0, 0, 0), (0, 0, 1), H, H, n, [s / m for s, m in zip(sV, n)], **kw)
    assert np.abs(mine - got).max() <= tol


def test_camera_refusals_and_the_orbit():
    ok = dict(eye=(3, 0, 0), target=(0, 0, 0), up=(0, 0, 1), H=4, W=6, sVoxel=(2, 2, 2), center=(0, 0, 0), nVoxel=(8, 8, 8))
    for kw in (dict(), dict(fov_y=30, ortho_height=2), dict(fov_y=180), dict(ortho_height=0), dict(fov_y=30, up=(1, 0, 0)),
               dict(fov_y=30, eye=(0, 0, 0)), dict(fov_y=30, H=0), dict(fov_y=30, sVoxel=(2, 2)), dict(fov_y=30, nVoxel=(8, 0, 8))):
        with pytest.raises(ValueError):
            VR.look_at_rays(**dict(ok, **kw))
    rays = VR.orbit_rays([0, 90, 180], 20.0, 3.0, 5, 7, (2, 2, 2), (0, 0, 0), (8, 8, 8))
    assert rays.shape == (3, 12) and rays.dtype == np.float32
    d = 2.0 / 8
    eye = (rays[:, :3] + 0.5) * d - 1.0                      # back from index units
    assert np.allclose(np.linalg.norm(eye, axis=1), 3.0, atol=1e-5) and np.allclose(eye[:, 2], 3.0 * math.sin(math.radians(20)), atol=1e-5)
    assert np.allclose(eye[1, :2], [0, 3.0 * math.cos(math.radians(20))], atol=1e-5)
    # square pixels: |pu| = |pv| in world units
    assert np.allclose(np.linalg.norm(rays[:, 6:9] * d, axis=1), np.linalg.norm(rays[:, 9:12] * d, axis=1), rtol=1e-6)


# ---- pictures ----------------------------------------------------------------------------------------------------------------------

def _png_chunks(data):
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    at, out = 8, []
    while at < len(data):
        size, kind = struct.unpack(">I4s", data[at:at + 8])
        body = data[at + 8:at + 8 + size]
        assert struct.unpack(">I", data[at + 8 + size:at + 12 + size])[0] == zlib.crc32(kind + body) & 0xFFFFFFFF
        out.append((kind, body))
        at += 12 + size
    return out


@pytest.mark.parametrize("shape", [(5, 7, 3), (4, 3), (1, 1, 3)])
def test_write_png_round_trips(tmp_path, shape):
    img = np.random.RandomState(2).randint(0, 256, shape).astype(np.uint8)
    path = str(tmp_path / "a.png")
    VR.write_png(path, img)
    chunks = _png_chunks(open(path, "rb").read())
    assert [k for k, _ in chunks] == [b"IHDR", b"IDAT", b"IEND"]
    W, H, depth, colour = struct.unpack(">IIBB", chunks[0][1][:10])
    assert (H, W, depth, colour) == (shape[0], shape[1], 8, 2 if len(shape) == 3 else 0)
    rows = np.frombuffer(zlib.decompress(chunks[1][1]), np.uint8).reshape(H, -1)
    assert (rows[:, 0] == 0).all() and np.array_equal(rows[:, 1:].reshape(shape), img)
    try:
        from PIL import Image
    except ImportError:
        return
    assert np.array_equal(np.asarray(Image.open(path)), img)


def test_write_png_refuses_other_arrays(tmp_path):
    for bad in (np.zeros((4, 4, 3), np.float32), np.zeros((4, 4, 4), np.uint8), np.zeros((0, 4, 3), np.uint8), np.zeros(4, np.uint8)):
        with pytest.raises(ValueError):
            VR.write_png(str(tmp_path / "b.png"), bad)


def test_over_and_to_rgb8():
    rgba = torch.tensor([[[0.25, 0.125, 0.0, 0.5], [0.0, 0.0, 0.0, 0.0], [1.0, 1.0, 1.0, 1.0]]])
    got = VR.over(rgba, (1.0, 0.0, 0.5))
    assert torch.allclose(got, torch.tensor([[[0.75, 0.125, 0.25], [1.0, 0.0, 0.5], [1.0, 1.0, 1.0]]]))
    assert VR.to_rgb8(got).tolist() == [[[191, 32, 64], [255, 0, 128], [255, 255, 255]]]
    assert VR.to_rgb8(np.array([-1.0, 2.0, np.nan, 0.5])).tolist() == [0, 255, 0, 128]
    with pytest.raises(ValueError):
        VR.over(rgba[..., :3])


def test_driver_defaults_are_plot_volumes():
    a = VR.parser().parse_args(["--volume", "v.npy", "--out", "o.png"])
    assert (a.cmap, a.opacity, a.clim, a.size, a.cut, a.mip, a.turntable) == ("viridis", "linear", [0.0, 1.0], [1000, 800], ["x", "0.5"], False, 0)
    # plot_volume.py's cpos about the centre of its 256^3 volume: the direction and distance of the eye
    e = np.array([-458.0015547298666, -207.26124611865254, 324.4699978427509]) - 128.0
    assert abs(math.degrees(math.atan2(e[1], e[0])) % 360 - a.azimuth) < 1 and abs(np.linalg.norm(e) / 256 - a.distance) < 0.05
    assert abs(math.degrees(math.asin(e[2] / np.linalg.norm(e))) - a.elevation) < 1 and a.fov == 30.0
    assert VR.default_unit([2.0, 2.0, 2.0], [256, 256, 256]) == pytest.approx(math.sqrt(12) / 256)


# ---- refusals ------------------------------------------------------------------------------------------------------------------------

def test_every_refusal_comes_before_the_library(monkeypatch):
    def no_library():
        raise AssertionError("the library was touched before the arguments were checked")
    monkeypatch.setattr(_lib, "lib", no_library)
    vol = torch.rand(4, 5, 6)
    rays = np.zeros((2, 12), np.float32)
    lut = R.ramp_lut(8, 1.0)
    ok = dict(vol=vol, rays=rays, cone=True, H=3, W=4, dVoxel=(0.1, 0.1, 0.1), lut=lut, clim=(0.0, 1.0))
    nan_lut, neg_lut = lut.copy(), lut.copy()
    nan_lut[3, 1], neg_lut[2, 3] = np.nan, -1.0
    for kw in (dict(H=0), dict(W=-1), dict(accuracy=0.0), dict(dVoxel=(0.1, 0.1)), dict(dVoxel=(0.1, 0.0, 0.1)),
               dict(lut=lut[:1]), dict(lut=np.zeros((1025, 4), np.float32)), dict(lut=lut[:, :3]), dict(lut=nan_lut),
               dict(lut=neg_lut), dict(clim=(1.0, 1.0)), dict(clim=(0.0, float("inf"))), dict(clim=(0.0,)),
               dict(t_stop=1.0), dict(t_stop=-0.1), dict(t_stop=float("nan"))):
        with pytest.raises(ValueError):
            VR.render_volume(**dict(ok, **kw))
    mok = dict(vol=vol, rays=rays, cone=True, H=3, W=4, dVoxel=(0.1, 0.1, 0.1))
    for kw in (dict(H=0), dict(accuracy=-1.0), dict(dVoxel=(1, 2))):
        with pytest.raises(ValueError):
            VR.mip(**dict(mok, **kw))
    # a host volume is refused next: the kernels have no CPU fallback
    for fn, args in ((VR.render_volume, ok), (VR.mip, mok), (VR.volume_bricks, dict(vol=vol)), (VR.picture, dict(vol=vol))):
        with pytest.raises(R2HipError):
            fn(**args)


def test_the_library_refuses_before_any_launch():
    """R2_ERR_INVALID comes back before the first launch, so these calls need no GPU: the pointers are never followed."""
    L = _lib.lib()
    p = 4096                                   # a stand-in for device pointers, 16-byte aligned
    names = ("V", "H", "W", "rays", "cone", "nx", "ny", "nz", "dx", "dy", "dz", "accuracy", "vol", "bricks", "K", "lut", "lo", "hi",
             "t_stop", "out")
    ok = dict(V=1, H=4, W=4, rays=p, cone=1, nx=4, ny=4, nz=4, dx=0.1, dy=0.1, dz=0.1, accuracy=0.5, vol=p, bricks=None, K=8, lut=p,
              lo=0.0, hi=1.0, t_stop=0.0, out=p)
    for change in (dict(K=1), dict(K=1025), dict(lut=None), dict(hi=0.0), dict(lo=1.0), dict(lo=float("-inf")),
                   dict(hi=float("inf")), dict(hi=float("nan")), dict(t_stop=1.0), dict(t_stop=-0.5), dict(t_stop=float("nan")),
                   dict(lut=p + 4), dict(out=p + 8), dict(bricks=p + 4), dict(V=0), dict(accuracy=0.0), dict(vol=None), dict(dx=0.0),
                   dict(V=65536)):
        a = dict(ok, **change)
        assert L.r2_render_volume(*[a[k] for k in names], None) == _lib.R2_ERR_INVALID, change
        assert L.r2_last_error()
    mnames = names[:14] + ("out",)
    for change in (dict(H=0), dict(accuracy=-1.0), dict(out=None), dict(bricks=p + 4), dict(nz=0)):
        a = dict(ok, **change)
        assert L.r2_render_volume_mip(*[a[k] for k in mnames], None) == _lib.R2_ERR_INVALID, change
    for args in ((0, 4, 4, p, p), (4, 4, 4, None, p), (4, 4, 4, p, None), (4, 4, 4, p, p + 4), (2 ** 31 - 1, 2 ** 20, 2 ** 20, p, p)):
        assert L.r2_volume_bricks(*args, None) == _lib.R2_ERR_INVALID, args
    assert _lib.R2_RENDER_BRICK == R.BRICK == 8
