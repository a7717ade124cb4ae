"""GPU: r2_volume_bricks, r2_render_volume and r2_render_volume_mip through volume_render.py against
tests/volume_render_ref.py -- the brick table and the MIP bit for bit, the compositing within 4 e32 + 8 u of float64 -- at the
shapes either side of a wave tile (8 x 8 pixels), a block (16 x 16), a brick (8 cells) and the table's limits (2 and 1024
rows); the same bits with and without the brick table; early termination; views alone and together; Beer-Lambert against
the device projector; the library's refusals; train.py --save_render and the driver."""
import os
import struct

import numpy as np
import pytest
import torch

from tests import volume_render_ref as R

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
NAMES = sorted(R.CASES)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def on_gpu(gpu, a):
    return torch.from_numpy(np.array(a)).to(gpu)      # a copy: the cases' arrays are read-only


def render(gpu, c, vol=None, **kw):
    from r2_gaussian_amd import volume_render as VR
    kw.setdefault("t_stop", 0.0)
    kw.setdefault("lut", c["lut"])
    v = on_gpu(gpu, c["vol"]) if vol is None else vol
    out = VR.render_volume(v, np.array(kw.pop("rays", c["rays"])), kw.pop("cone", c["cone"]), c["H"], c["W"], c["dVoxel"],
                           clim=c["clim"], accuracy=c["accuracy"], **kw)
    assert out.dtype == torch.float32 and out.shape[1:] == (c["H"], c["W"], 4)
    return out.cpu().numpy().reshape(-1, 4)


def mip(gpu, c, vol=None, **kw):
    from r2_gaussian_amd import volume_render as VR
    v = on_gpu(gpu, c["vol"]) if vol is None else vol
    out = VR.mip(v, np.array(kw.pop("rays", c["rays"])), kw.pop("cone", c["cone"]), c["H"], c["W"], c["dVoxel"], accuracy=c["accuracy"], **kw)
    return out.cpu().numpy().reshape(-1)


# ---- 1: the brick table and the MIP, bit for bit -------------------------------------------------------------------------------

@pytest.mark.parametrize("name", NAMES)
def test_bricks_and_mip_are_the_restatement(gpu, name):
    from r2_gaussian_amd import volume_render as VR
    c = R.case(name)
    table = VR.volume_bricks(on_gpu(gpu, c["vol"]))
    assert same_bits(table.cpu().numpy(), R.bricks(c["vol"]))
    want = R.mip(c["walk"])
    assert same_bits(mip(gpu, c, bricks=False), want)
    assert same_bits(mip(gpu, c, bricks=True), want)
    assert same_bits(mip(gpu, c, bricks=table), want)
    assert (want[~c["walk"]["hit"]] == 0).all()


@pytest.mark.parametrize("shape", [(1, 1, 1), (2, 7, 9), (5, 8, 17), (25, 15, 16), (17, 2, 8)])
def test_bricks_at_the_edges_of_a_brick(gpu, shape):
    from r2_gaussian_amd import volume_render as VR
    vol = np.random.RandomState(sum(shape)).uniform(-1.0, 1.0, shape).astype(np.float32)
    vol[vol > 0.9] = 0.0
    vol.ravel()[0] = -0.0
    got = VR.volume_bricks(on_gpu(gpu, vol)).cpu().numpy()
    assert got.shape == tuple((n + 7) // 8 for n in shape) + (2,) and same_bits(got, R.bricks(vol))


# ---- 2: the compositing against float64 ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", NAMES)
def test_render_is_within_the_measured_float32_error(gpu, name):
    c = R.case(name)
    e32 = R.load_e32()[name]
    got = render(gpu, c, bricks=False)
    _, want = R.reference(name)
    err = np.abs(got.astype(np.float64) - want).max(0)
    tol = 4 * e32 + 8 * U
    print("%s: worst |gpu - f64| per channel %s, e32 %.3e, worst ratio to 4 e32 + 8 u: %.3f"
          % (name, " ".join("%.3e" % e for e in err), e32, err.max() / tol))
    assert (err <= tol).all()
    assert (got[~c["walk"]["hit"]] == 0).all() and not np.signbit(got[~c["walk"]["hit"]]).any()


# ---- 3: the same bits with and without the table ----------------------------------------------------------------------------------

def _sparse_views():
    """Rays through the sparse volume that make the jump work hardest: parallel views along +x, -y and +z whose pixel points
    are integers, so that rays lie exactly on brick faces (8, 16, 24) with two zero direction components; and a cone source
    inside the volume."""
    par = np.array([[1, 0, 0, -4, -2, -2, 0, 2, 0, 0, 0, 2],
                    [0, -1, 0, -2, 30, -2, 2, 0, 0, 0, 0, 2],
                    [0, 0, 1, -2, -2, -7.5, 0, 2, 0, 2, 0, 0]], np.float32)
    c = R.case("sparse_blobs")
    cone, _ = R.camera_rays((0.1, -0.05, 0.02), (-0.4, -0.3, -0.45), (0, 0, 1), c["H"], c["W"], c["vol"].shape, c["dVoxel"], fov_y=100.0)
    return par, cone


@pytest.mark.parametrize("name", NAMES)
def test_the_brick_table_changes_no_bit(gpu, name):
    from r2_gaussian_amd import volume_render as VR
    c = R.case(name)
    vol = on_gpu(gpu, c["vol"])
    table = VR.volume_bricks(vol)
    K = len(c["lut"])
    window = c["lut"].copy()
    window[: max(1, (3 * K) // 5), 3] = 0.0          # a second table, transparent below 60 % of the window
    for lut in (c["lut"], window):
        for t_stop in (0.0, 2.0 ** -10):
            off = render(gpu, c, vol, lut=lut, t_stop=t_stop, bricks=False)
            assert same_bits(render(gpu, c, vol, lut=lut, t_stop=t_stop, bricks=True), off)
            assert same_bits(render(gpu, c, vol, lut=lut, t_stop=t_stop, bricks=table), off)
    assert same_bits(mip(gpu, c, vol, bricks=table), mip(gpu, c, vol, bricks=None))


@pytest.mark.parametrize("K", [2, 3, 256, 1024])
def test_skipping_runs_and_changes_no_bit(gpu, K):
    """The sparse volume under the "linear" ramp: most bricks test empty by the restatement's table, so the jump runs; every
    table size, parallel rays on brick faces, a source inside, V = 3 and V = 1."""
    c = R.case("sparse_blobs")
    lut = R.ramp_lut(K, 0.1)
    empty = R.empty_bricks(R.bricks(c["vol"]), lut, *c["clim"])
    print("K %d: %d of %d bricks empty" % (K, empty.sum(), empty.size))
    assert empty.mean() >= 0.5
    vol = on_gpu(gpu, c["vol"])
    par, cone = _sparse_views()
    for rays, is_cone in ((c["rays"], True), (par, False), (par[1:2], False), (cone, True)):
        for t_stop in (0.0, 2.0 ** -10):
            off = render(gpu, c, vol, rays=rays, cone=is_cone, lut=lut, t_stop=t_stop, bricks=False)
            on = render(gpu, c, vol, rays=rays, cone=is_cone, lut=lut, t_stop=t_stop, bricks=True)
            assert same_bits(on, off) and off[:, 3].max() > 0
        assert same_bits(mip(gpu, c, vol, rays=rays, cone=is_cone, bricks=True), mip(gpu, c, vol, rays=rays, cone=is_cone, bricks=False))
    # and the skipped picture is still the restatement's: the float64 reference of the named case (K = 256)
    if K == 256:
        got = render(gpu, c, vol, lut=lut, bricks=True)
        assert np.abs(got - R.reference("sparse_blobs")[1]).max() <= 4 * R.load_e32()["sparse_blobs"] + 8 * U


# ---- 4: early termination ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("t_stop", [2.0 ** -10, 0.25])
def test_early_termination_moves_no_channel_by_more_than_t_stop(gpu, name, t_stop):
    c = R.case(name)
    e32 = R.load_e32()[name]
    vol = on_gpu(gpu, c["vol"])
    full = render(gpu, c, vol).astype(np.float64)
    cut = render(gpu, c, vol, t_stop=t_stop).astype(np.float64)
    moved = np.abs(full - cut)
    left = 1.0 - cut[:, 3]                                        # T of the shortened ray, up to the rounding of 1 - T
    stopped = left < t_stop + 2 * U
    print("%s t_stop %g: %d of %d rays stopped, moved at most %.3e" % (name, t_stop, stopped.sum(), len(cut), moved.max()))
    assert moved.max() <= t_stop + 4 * e32
    assert (moved[stopped] <= left[stopped, None] + 4 * e32 + 8 * U).all()   # what is left behind is at most T (colours <= 1)
    assert (moved[left > t_stop + 2 * U] == 0).all()              # a ray that never fell below t_stop is untouched


# ---- 5: views alone, repeated runs, the input --------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["dense_orbit", "partial_miss"])
def test_a_view_alone_is_the_view_among_three(gpu, name):
    c = R.case(name)
    assert len(c["rays"]) == 3
    vol = on_gpu(gpu, c["vol"])
    before = vol.clone()
    per = c["H"] * c["W"]
    for kw in (dict(bricks=True), dict(bricks=False, t_stop=0.125)):
        together = render(gpu, c, vol, **kw)
        assert same_bits(render(gpu, c, vol, **kw), together)
        for v in range(3):
            assert same_bits(render(gpu, c, vol, rays=c["rays"][v:v + 1], **kw), together[v * per:(v + 1) * per])
    m = mip(gpu, c, vol)
    for v in range(3):
        assert same_bits(mip(gpu, c, vol, rays=c["rays"][v:v + 1]), m[v * per:(v + 1) * per])
    assert torch.equal(vol, before)


def test_out_is_written_in_place(gpu):
    from r2_gaussian_amd import volume_render as VR
    c = R.case("single_voxel")
    vol = on_gpu(gpu, c["vol"])
    out = torch.full((1, c["H"], c["W"], 4), 7.0, device=gpu)
    got = VR.render_volume(vol, c["rays"], c["cone"], c["H"], c["W"], c["dVoxel"], c["lut"], c["clim"], t_stop=0.0, out=out)
    assert got is out and same_bits(out.cpu().numpy().reshape(-1, 4), render(gpu, c, vol))
    for bad in (out[..., :3], out.double(), out.cpu(), out[:, :, :-1]):
        with pytest.raises(ValueError):
            VR.render_volume(vol, c["rays"], c["cone"], c["H"], c["W"], c["dVoxel"], c["lut"], c["clim"], out=bad)
    with pytest.raises(ValueError):
        VR.render_volume(vol, c["rays"], c["cone"], c["H"], c["W"], c["dVoxel"], c["lut"], c["clim"], bricks=torch.zeros(2, 1, 1, 2, device=gpu))


# ---- 6: Beer-Lambert against the device projector --------------------------------------------------------------------------------

def test_beer_lambert_against_the_device_projector(gpu):
    """The beer_lambert case's table has colour 1 and an extinction kappa * value: alpha = 1 - exp(-kappa * line integral), the
    line integral being projector.project_rays' over the same samples."""
    from r2_gaussian_amd import projector as PJ
    c = R.case("beer_lambert")
    e32 = R.load_e32()["beer_lambert"]
    vol = on_gpu(gpu, c["vol"])
    got = render(gpu, c, vol).astype(np.float64)
    line = PJ.project_rays(vol, c["rays"], c["cone"], c["H"], c["W"], c["dVoxel"], c["accuracy"]).cpu().numpy().reshape(-1)
    want = 1.0 - np.exp(-R.KAPPA * line.astype(np.float64))
    err = np.abs(got[:, 3] - want).max()
    print("Beer-Lambert: worst |alpha - (1 - exp(-kappa P))| %.3e, e32 %.3e, ratio %.3f" % (err, e32, err / e32))
    assert err <= e32
    # colour 1: C = sum T_k (1 - e_k) telescopes to 1 - T.  In float32 C takes n sums and T n products, each rounded by at most
    # u relative to a value <= 1, and each term two more roundings: (2 n + 2) u in all
    n = int(c["walk"]["n"].max())
    drift = np.abs(got[:, :3] - got[:, 3:4]).max()
    print("C against 1 - T: %.3e, (2 n + 2) u = %.3e at n = %d" % (drift, (2 * n + 2) * U, n))
    assert drift <= (2 * n + 2) * U
    assert want.max() > 0.5


# ---- 7: the library's refusals ---------------------------------------------------------------------------------------------------

def test_the_library_refuses_each_limit_and_writes_nothing(gpu):
    from r2_gaussian_amd import _boundary, _lib
    from r2_gaussian_amd.projector import device_rays
    c = R.case("single_voxel")
    vol, lut, rays = on_gpu(gpu, c["vol"]), on_gpu(gpu, c["lut"]), device_rays(c["rays"], gpu)
    out = torch.full((1, c["H"], c["W"], 4), 7.0, device=gpu)
    names = ("V", "H", "W", "rays", "cone", "nx", "ny", "nz", "dx", "dy", "dz", "accuracy", "vol", "bricks", "K", "lut", "lo", "hi",
             "t_stop", "out")
    ok = dict(V=1, H=c["H"], W=c["W"], rays=rays, cone=1, nx=1, ny=1, nz=1, dx=0.5, dy=0.4, dz=0.3, accuracy=0.5, vol=vol,
              bricks=None, K=3, lut=lut, lo=0.0, hi=1.0, t_stop=0.0, out=out)
    big = torch.zeros(1025 * 4, device=gpu)
    for change in (dict(K=1), dict(K=1025, lut=big), dict(hi=0.0), dict(lo=float("nan")), dict(hi=float("inf")), dict(t_stop=1.0),
                   dict(t_stop=-0.25), dict(lut=None), dict(accuracy=0.0), dict(V=0), dict(V=65536), dict(dz=0.0), dict(vol=None),
                   dict(lut=big[1:13]), dict(out=out.view(-1)[1:])):
        a = dict(ok, **change)
        with pytest.raises(_lib.R2HipError, match=str(_lib.R2_ERR_INVALID)):
            _boundary.call("r2_render_volume", gpu, *[a[k] for k in names])
    flat = torch.full((1, c["H"], c["W"]), 7.0, device=gpu)
    for change in (dict(H=0), dict(accuracy=float("nan")), dict(rays=None)):
        a = dict(ok, out=flat, **change)
        with pytest.raises(_lib.R2HipError, match=str(_lib.R2_ERR_INVALID)):
            _boundary.call("r2_render_volume_mip", gpu, *[a[k] for k in names[:14] + ("out",)])
    with pytest.raises(_lib.R2HipError, match=str(_lib.R2_ERR_INVALID)):
        _boundary.call("r2_volume_bricks", gpu, 1, 0, 1, vol, flat)
    torch.cuda.synchronize(gpu)
    assert bool((out == 7.0).all()) and bool((flat == 7.0).all())
    _boundary.call("r2_render_volume", gpu, *[ok[k] for k in names])   # and the unchanged arguments are accepted
    assert bool((out != 7.0).all())


# ---- 8: train.py --save_render and the driver --------------------------------------------------------------------------------------

def _png_size(path):
    with open(path, "rb") as f:
        head = f.read(26)
    assert head[:8] == b"\x89PNG\r\n\x1a\n" and head[12:16] == b"IHDR"
    W, H, depth, colour = struct.unpack(">IIBB", head[16:26])
    assert (depth, colour) == (8, 2)
    return H, W


def test_save_render_and_the_command_line(gpu, tmp_path, capsys):
    """train.py --save_render on the tiny case of the --save_mesh test, then python -m r2_gaussian_amd.volume_render on its
    ground-truth volume (both mains in this process): PNGs of the requested sizes."""
    from r2_gaussian_amd import datagen as D
    from r2_gaussian_amd import scene as S
    from r2_gaussian_amd import train as TR
    from r2_gaussian_amd import volume_render as VR
    from tests.test_isosurface_gpu import _blob
    n, iters = 32, 20
    vol = _blob(n, (0.1, -0.2, 0.05), 0.3, 0.6) + _blob(n, (-0.3, 0.25, -0.1), 0.15, 0.5)
    cfg = dict(S.CONE_BEAM, nVoxel=[n, n, n], nDetector=[64, 64], noise=False, totalAngle=360.0, startAngle=0.0)
    case = D.generate(vol, cfg, str(tmp_path / "data"), "phantom", n_train=12, n_test=2, seed=0)
    out = str(tmp_path / "out")
    TR.main(["-s", case, "-m", out, "--iterations", str(iters), "--test_iterations", str(iters), "--quiet", "--save_render", "50", "40"])
    pc = os.path.join(out, "point_cloud", "iteration_%d" % iters)
    assert _png_size(os.path.join(pc, "render.png")) == (50, 40)
    meta = os.path.join(case, "meta_data.json")
    VR.main(["--volume", os.path.join(case, "vol_gt.npy"), "--meta", meta, "--out", str(tmp_path / "volume.png"), "--size", "45", "36"])
    assert _png_size(str(tmp_path / "volume.png")) == (45, 36)
    assert "volume.png: 36 x 45" in capsys.readouterr().out
    # the half-cut picture shows the phantom: not one flat background
    from tests.test_volume_render_cpu import _png_chunks
    import zlib
    rows = np.frombuffer(zlib.decompress(_png_chunks(open(str(tmp_path / "volume.png"), "rb").read())[1][1]), np.uint8).reshape(45, -1)
    assert rows[:, 1:].min() < 200 and rows[0, 1:4].min() > 250
    VR.main(["--volume", os.path.join(pc, "vol_pred.npy"), "--out", str(tmp_path / "turn.png"), "--size", "17", "9", "--mip",
             "--turntable", "2", "--cmap", "gray", "--cut", "z", "0"])
    assert _png_size(str(tmp_path / "turn_000.png")) == (17, 9) and _png_size(str(tmp_path / "turn_001.png")) == (17, 9)
