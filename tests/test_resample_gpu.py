"""Cubic-spline resampling on the MI355X (csrc/spline.hip, r2_gaussian_amd/resample.py, prepare.py): the prefilter, the zoom
and the sampler bit for bit against the float32 restatement (tests/resample_ref.py), identities on the device, reshape_vol
against scipy's fixtures, the raw-data driver through to a generated case, and validation before any launch."""
import os

import numpy as np
import pytest
import torch

from r2_gaussian_amd import _lib
from r2_gaussian_amd import prepare as PR
from r2_gaussian_amd import resample as RS
from r2_gaussian_amd._boundary import call
from r2_gaussian_amd._lib import R2HipError
from tests import resample_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "resample")

# The issue's shapes with their factors, then the kernels' tile edges (csrc/spline.hip).  The z pass moves ZT_CHUNK = 64
# elements of a padded line (n + 24) at a time: nz = 40, 41 and 103 give padded lines of exactly one chunk, one element more
# than one chunk and one less than two.  Its workgroups take ZT_LINES = 64 lines and the x / y passes TB = 256 lines of the
# padded block, which has at least 25 * 25 = 625 of them along every axis, so every shape has a partial last workgroup and
# several full ones: (1, 1, 1) has 625 lines (9 full z workgroups and 49 lines; 2 full x / y workgroups and 113 lines).  The
# zoom has TB = 256 outputs per workgroup: the factors of (2, 3, 41) give 257 and 511 outputs.  (1, 2, 103) and (90, 1, 1)
# hold zeros from their ninth sample on: the recursion decays through the denormal range there.
EDGE_CASES = [
    ((3, 1, 40), [(1.4, 2.0, 0.6)]),
    ((2, 3, 41), [(0.5, 0.4, 257 / 41), (0.5, 7 / 3, 73 / 41), 1.0]),
    ((1, 2, 103), [(1.0, 1.5, 0.33), (3.0, 0.5, 1.1)]),
    ((90, 1, 1), [(0.5, 2.0, 2.0), (1.2, 1.0, 1.0)]),
]
CASES = R.ZOOM_CASES + EDGE_CASES
_IDS = ["x".join(map(str, s)) for s, _ in CASES]


def _volume(shape):
    v = R.case_volume(shape)
    if shape in ((1, 2, 103), (90, 1, 1)):
        v.reshape(-1 if shape[0] == 90 else 2, max(shape))[..., 8:] = 0.0
    return v


def _bits_equal(got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    return got.dtype == want.dtype == np.float32 and got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32))


_COEFFS = {}


def _coeffs32(shape):
    """The float32 restatement's coefficients of a case's volume: computed once, shared, never written."""
    if shape not in _COEFFS:
        c = R.prefilter(_volume(shape), np.float32)
        c.setflags(write=False)
        _COEFFS[shape] = c
    return _COEFFS[shape]


@pytest.mark.parametrize("shape,factors", CASES, ids=_IDS)
def test_prefilter_and_zoom_equal_the_float32_restatement_bit_for_bit(gpu, shape, factors):
    vol = _volume(shape)
    v = torch.from_numpy(vol).to(gpu)
    want_c = _coeffs32(shape)
    if shape in ((1, 2, 103), (90, 1, 1)):
        tiny = np.abs(want_c[want_c != 0]).min()
        assert tiny < np.finfo(np.float32).tiny, tiny    # the case does reach the denormals
    got_c = RS.spline_filter(v).cpu().numpy()
    assert got_c.shape == tuple(n + 24 for n in shape)
    assert _bits_equal(got_c, want_c), float(np.abs(got_c.astype(np.float64) - want_c).max())
    assert np.array_equal(v.cpu().numpy(), vol)                         # the input is untouched
    for f in factors:
        want = R.zoom_coeffs(want_c, shape, R.out_shape(shape, f), np.float32)
        got = RS.zoom(v, f).cpu().numpy()
        assert _bits_equal(got, want), (f, got.shape, want.shape)


def _points(shape, n):
    """n float32 points: the fixture's (lattice nodes, the ends of the padded block and beyond), filled up with random ones;
    one NaN and one infinite coordinate once there is room."""
    base = R.case_points(shape, n_random=40)
    rng = np.random.RandomState(n)
    extra = (rng.rand(max(n - len(base), 0), 3) * (np.array(shape) + 30) - 15).astype(np.float32)
    p = np.concatenate([base, extra])[-n:] if n else np.zeros((0, 3), np.float32)
    if n >= 65:
        p[3, 1] = np.nan
        p[n - 2, 2] = np.inf
        p[n // 2, 0] = -np.inf
    return p


@pytest.mark.parametrize("shape", [(6, 5, 7), (2, 3, 1), (1, 1, 1), (2, 3, 41)], ids=str)
def test_sampler_equals_the_float32_restatement_bit_for_bit(gpu, shape):
    v = torch.from_numpy(_volume(shape)).to(gpu)
    coeffs = RS.spline_filter(v)
    want_c = _coeffs32(shape)
    for n in (0, 1, 65, 257, 4097):
        p = _points(shape, n)
        want = R.sample_coeffs(want_c, shape, p, np.float32)
        got = RS.map_coordinates(coeffs, torch.from_numpy(p).to(gpu), prefiltered=True).cpu().numpy()
        bad = ~np.isfinite(p).all(axis=1)
        assert got.shape == (n,) and np.array_equal(np.isnan(got), bad) and int(bad.sum()) == (3 if n >= 65 else 0)
        assert _bits_equal(got[~bad], want[~bad]), n
    # from the volume itself, and for any leading shape
    p = _points(shape, 24)
    got = RS.map_coordinates(v, torch.from_numpy(p.reshape(2, 3, 4, 3)).to(gpu))
    assert got.shape == (2, 3, 4) and _bits_equal(got.cpu().numpy().reshape(-1), R.sample_coeffs(want_c, shape, p, np.float32))


def test_sampler_against_scipys_fixture(gpu):
    for shape in R.SAMPLE_SHAPES:
        d = np.load(os.path.join(GOLD, "sample_%s.npz" % "x".join(map(str, shape))))
        got = RS.map_coordinates(torch.from_numpy(d["vol"]).to(gpu), torch.from_numpy(d["points"]).to(gpu)).cpu().numpy()
        assert float(np.abs(got - d["values"]).max()) < R.F32_BOUND
    # on the lattice nodes the spline interpolates the volume
    vol = _volume((7, 5, 9))
    nodes = np.stack(np.meshgrid(*[np.arange(k) for k in vol.shape], indexing="ij"), -1).astype(np.float32)
    got = RS.map_coordinates(torch.from_numpy(vol).to(gpu), torch.from_numpy(nodes).to(gpu)).cpu().numpy()
    assert got.shape == vol.shape and float(np.abs(got - vol).max()) < R.F32_BOUND


def test_identities_on_the_device(gpu):
    shape = (7, 5, 9)
    vol = _volume(shape)
    v = torch.from_numpy(vol).to(gpu)
    a = RS.zoom(v, 1.7)
    assert torch.equal(RS.zoom(v, 1.7), a) and torch.equal(RS.spline_filter(v), RS.spline_filter(v))      # two runs
    assert torch.equal(v.cpu(), torch.from_numpy(vol))
    out = torch.full((12, 8, 15), float("nan"), device=gpu)
    assert RS.zoom(v, 1.7, out=out) is out and torch.equal(out, a)                                          # NaN-filled out
    # NaN-filled coefficients' buffer and an oversized NaN-filled workspace, through the C ABI
    coeffs = torch.full((31, 29, 33), float("nan"), device=gpu)
    call("r2_spline_prefilter", gpu, 7, 5, 9, v, coeffs)
    assert torch.equal(coeffs, RS.spline_filter(v))
    nbytes = int(_lib.lib().r2_spline_zoom_workspace_bytes(12, 8, 15))
    assert nbytes == (12 + 8 + 15) * 20
    ws = torch.full((nbytes // 4 + 1000,), float("nan"), device=gpu)
    out.fill_(float("nan"))
    call("r2_spline_zoom", gpu, 7, 5, 9, coeffs, 12, 8, 15, out, ws, ws.numel() * 4)
    assert torch.equal(out, a)
    # the passes one by one are the whole
    c2 = torch.full_like(coeffs, float("nan"))
    for axis in range(3):
        call("r2_spline_prefilter_pass", gpu, 7, 5, 9, v if axis == 0 else None, c2, axis)
    assert torch.equal(c2, coeffs)
    # a factor of 1 filters and evaluates the spline again, as scipy does: the restatement, not a copy
    one = RS.zoom(v, 1.0).cpu().numpy()
    assert _bits_equal(one, R.zoom(vol, 1.0, np.float32)) and float(np.abs(one - vol).max()) < R.F32_BOUND
    # ... while resize with every factor 1 returns its input
    cube = torch.from_numpy(_volume((6, 6, 6))).to(gpu)
    assert RS.resize(cube, 6) is cube
    assert RS.resize(cube, 9).shape == (9, 9, 9)
    # other dtypes and layouts are converted
    assert torch.equal(RS.zoom(v.double(), 1.7), a)
    assert torch.equal(RS.zoom(v.permute(2, 1, 0), 1.3), RS.zoom(v.permute(2, 1, 0).contiguous(), 1.3))
    # the cube helpers
    e = RS.expand_to_cube(v).cpu().numpy()
    assert np.array_equal(e, R.expand_to_cube(vol))
    assert np.array_equal(RS.crop_to_cube(v).cpu().numpy(), R.crop_to_cube(vol))
    r, sp = RS.resample(v, (1.3, 0.8, 1.1))
    want, sp_want = R.resample(vol, (1.3, 0.8, 1.1), zoom_fn=R.zoom32)
    assert _bits_equal(r.cpu().numpy(), want) and np.array_equal(sp, sp_want)


def test_no_host_sync(gpu):
    v = torch.from_numpy(_volume((7, 5, 9))).to(gpu)
    p = torch.from_numpy(_points((7, 5, 9), 65)).to(gpu)
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        a = RS.zoom(v, (1.7, 0.5, 1.2))
        b = RS.map_coordinates(v, p)
        c = RS.reshape_vol(v, (1.3, 0.8, 1.1), 8, "expand")
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    assert a.shape == (12, 2, 11) and b.shape == (65,) and c.shape == (8, 8, 8)


@pytest.mark.parametrize("mode", [None, "crop", "expand"], ids=str)
def test_reshape_vol_against_the_fixtures(gpu, mode):
    d = np.load(os.path.join(GOLD, "reshape_%s.npz" % mode))
    got = RS.reshape_vol(torch.from_numpy(d["vol"]).to(gpu), d["spacing"], int(d["target"]), mode).cpu().numpy()
    assert got.shape == (8, 8, 8)
    assert float(np.abs(got - d["out"]).max()) < R.F32_BOUND
    assert _bits_equal(got, R.reshape_vol(d["vol"], d["spacing"], int(d["target"]), mode, R.zoom32))
    with pytest.raises(ValueError):
        RS.reshape_vol(torch.from_numpy(d["vol"]).to(gpu), d["spacing"], 8, "pad")


def test_raw_file_to_a_generated_case(gpu, tmp_path):
    import yaml
    from r2_gaussian_amd import datagen as D
    shape = [6, 5, 7]
    raw = np.random.RandomState(3).randint(0, 4000, size=shape[::-1]).astype(np.uint16)
    raw.tofile(str(tmp_path / "scan.raw"))
    info = [dict(raw_path=str(tmp_path / "scan.raw"), output_name="0_scan", file_type="raw", dtype="uint16", shape=shape,
                 spacing=[1.0, 1.2, 0.9], reshape="expand", transpose=[1, 0, 2], z_invert=True)]
    with open(str(tmp_path / "meta.yml"), "w") as f:
        yaml.safe_dump(info, f)
    out = str(tmp_path / "volume_gt")
    PR.main(["--metadata", str(tmp_path / "meta.yml"), "--output", out, "--target_size", "16"])
    got = np.load(os.path.join(out, "0_scan.npy"))
    data = raw.astype(float).transpose(2, 1, 0)
    data = ((data - data.min()) / (data.max() - data.min())).clip(0.0, 1.0)
    want = R.reshape_vol(data.astype(np.float32), [1.0, 1.2, 0.9], 16, "expand", R.zoom32).clip(0.0, 1.0)
    assert got.dtype == np.float32 and np.array_equal(got, want.transpose(1, 0, 2)[:, :, ::-1])
    with open(os.path.join(ROOT, "tests", "golden", "scanner", "cone_beam.yml")) as f:
        cfg = yaml.safe_load(f)
    cfg.update(nVoxel=[16, 16, 16], nDetector=[24, 24])
    with open(str(tmp_path / "scanner.yml"), "w") as f:
        yaml.safe_dump(cfg, f)
    case = D.main(["--vol", os.path.join(out, "0_scan.npy"), "--scanner", str(tmp_path / "scanner.yml"), "--output",
                   str(tmp_path / "data"), "--n_train", "4", "--n_test", "2"])
    assert os.path.basename(case) == "0_scan_cone" and np.array_equal(np.load(os.path.join(case, "vol_gt.npy")), got)


def test_validation_before_any_launch(gpu):
    v = torch.rand(4, 5, 6, device=gpu)
    coeffs = torch.full((28, 29, 30), 7.0, device=gpu)
    out = torch.full((3, 4, 5), 7.0, device=gpu)
    pts = torch.zeros(5, 3, device=gpu)
    vals = torch.full((5,), 7.0, device=gpu)
    nbytes = int(_lib.lib().r2_spline_zoom_workspace_bytes(3, 4, 5))
    ws = torch.full((nbytes // 4,), 7.0, device=gpu)
    big = 2 ** 31 - 1
    bad = [("r2_spline_prefilter", (0, 5, 6, v, coeffs)), ("r2_spline_prefilter", (4, -1, 6, v, coeffs)),
           ("r2_spline_prefilter", (4, 5, 6, None, coeffs)), ("r2_spline_prefilter", (4, 5, 6, v, None)),
           ("r2_spline_prefilter", (1300, 1300, 1300, v, coeffs)), ("r2_spline_prefilter", (big, big, big, v, coeffs)),
           ("r2_spline_prefilter_pass", (4, 5, 6, v, coeffs, 3)), ("r2_spline_prefilter_pass", (4, 5, 6, v, coeffs, -1)),
           ("r2_spline_prefilter_pass", (4, 5, 6, None, coeffs, 0)), ("r2_spline_prefilter_pass", (4, 5, 6, v, None, 1)),
           ("r2_spline_zoom", (4, 5, 6, coeffs, 0, 4, 5, out, ws, nbytes)), ("r2_spline_zoom", (4, 5, 0, coeffs, 3, 4, 5, out, ws, nbytes)),
           ("r2_spline_zoom", (4, 5, 6, None, 3, 4, 5, out, ws, nbytes)), ("r2_spline_zoom", (4, 5, 6, coeffs, 3, 4, 5, None, ws, nbytes)),
           ("r2_spline_zoom", (4, 5, 6, coeffs, 3, 4, 5, out, None, nbytes)),
           ("r2_spline_zoom", (4, 5, 6, coeffs, 3, 4, 5, out, ws, nbytes - 1)),
           ("r2_spline_zoom", (4, 5, 6, coeffs, 2048, 2048, 512, out, ws, 2 ** 40)),
           ("r2_spline_zoom", (1300, 1300, 1300, coeffs, 3, 4, 5, out, ws, nbytes)),
           ("r2_spline_sample", (4, 5, 6, None, 5, pts, vals)), ("r2_spline_sample", (4, 5, 6, coeffs, 5, None, vals)),
           ("r2_spline_sample", (4, 5, 6, coeffs, 5, pts, None)), ("r2_spline_sample", (4, 5, 6, coeffs, -1, pts, vals)),
           ("r2_spline_sample", (4, 0, 6, coeffs, 5, pts, vals))]
    for name, args in bad:
        with pytest.raises(R2HipError):
            call(name, gpu, *args)
    assert call("r2_spline_sample", gpu, 4, 5, 6, coeffs, 0, None, None) == 0                   # N = 0: a no-op
    assert RS.map_coordinates(v, torch.zeros(0, 3, device=gpu)).shape == (0,)
    # the Python surface
    for fn, args in ((RS.zoom, (v[0], 2.0)), (RS.zoom, (v, (2.0, 1.0))), (RS.zoom, (v, 0.01)),
                     (RS.zoom, (v, 2.0, torch.empty(8, 10, 11, device=gpu))),
                     (RS.zoom, (v, 2.0, torch.empty(8, 10, 12, device=gpu).double())), (RS.spline_filter, (v.reshape(1, 4, 5, 6),)),
                     (RS.map_coordinates, (v, torch.zeros(5, 2, device=gpu))), (RS.map_coordinates, (v, torch.zeros(5, 3, device=gpu), True))):
        with pytest.raises(ValueError):
            fn(*args)
    for fn, args in ((RS.zoom, (v.cpu(), 2.0)), (RS.zoom, (v, 2.0, torch.empty(8, 10, 12))), (RS.map_coordinates, (v, pts.cpu())),
                     (RS.map_coordinates, (v, pts.cpu().numpy()))):
        with pytest.raises(R2HipError):
            fn(*args)
    torch.cuda.synchronize()
    for t in (coeffs, out, vals, ws):
        assert bool((t == 7.0).all())   # nothing was launched into them
