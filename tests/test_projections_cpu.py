"""CPU: the restatement of the projection-conditioning kernels (tests/projections_ref.py) against independent implementations
-- its own float64 run, torch's bilinear interpolate, a reshape-mean, scipy's median filter -- the NaN rules against hand-built
cases, the host logic of prepare_real.py, and the refusals that need no GPU.  The kernels themselves are pinned to the
restatement bit for bit in tests/test_projections_gpu.py."""
import random

import numpy as np
import pytest
import scipy.ndimage as ndimage
import torch

from r2_gaussian_amd import _lib
from r2_gaussian_amd import prepare_real as PR
from r2_gaussian_amd import projections as PJ
from r2_gaussian_amd._lib import R2HipError
from tests import projections_ref as R

U = 2.0 ** -24   # the unit roundoff of float32

_SHAPE_IDS = ["%dx%d-%dx%d" % (s + m) for s, m in R.RESIZE_SHAPES]


@pytest.mark.parametrize("shape,size", R.RESIZE_SHAPES, ids=_SHAPE_IDS)
def test_linear_float32_against_float64_on_the_same_weights(shape, size):
    """Two stages of two products and a sum: each product and each sum adds at most u times a value of at most M = max|P|
    (the weights of a stage are non-negative and sum to 1 within u), 4 u M in all plus second-order terms: asserted at 5 u M."""
    for lo, shift in ((None, (0, 0)), (0.0, (5, 0)), (None, (-2, 3))):
        src = R.case_stack(2, shape)
        got = R.resize_linear(src, size, shift, lo, dtype=np.float32)
        want = R.resize_linear(src, size, shift, lo, dtype=np.float64)
        assert got.dtype == np.float32 and want.dtype == np.float64 and got.shape == (2,) + size
        M = float(np.abs(R.prepared(src, shift, lo)).max())
        err = float(np.abs(got.astype(np.float64) - want).max())
        print("float32 vs float64:", shape, size, shift, lo, "error %.3g = %.2f u M" % (err, err / (U * M) if M else 0.0))
        assert err <= 5 * U * M


@pytest.mark.parametrize("shape,size", R.RESIZE_SHAPES, ids=_SHAPE_IDS)
def test_linear_float64_against_torch_bilinear(shape, size):
    """torch's bilinear interpolate with align_corners=False samples by the same rule, in float64 throughout.  The restatement
    rounds the source coordinate, which is below n, to float32: a weight moves by at most n 2^-24 per axis, the result by at most
    2 n 2^-24 (max - min); asserted at twice that, n_max 2^-22 (max - min)."""
    src = R.case_stack(2, shape, seed=1)
    got = R.resize_linear(src, size, dtype=np.float64)
    want = torch.nn.functional.interpolate(torch.from_numpy(src.astype(np.float64))[None], size=size, mode="bilinear",
                                           align_corners=False)[0].numpy()
    err = float(np.abs(got - want).max())
    bound = max(shape) * 2.0 ** -22 * float(src.max() - src.min())
    print("float64 vs torch:", shape, size, "error %.3g, bound %.3g" % (err, bound))
    assert err <= bound


def test_linear_tables_at_the_borders():
    s, f = R.linear_table(6, 13)            # an upscale: the first source coordinate is negative
    assert s[0] == 0 and f[0] == 0 and s[-1] == 5 and f[-1] == 0 and (f >= 0).all() and (f < 1).all()
    s, f = R.linear_table(1, 4)
    assert (s == 0).all() and (f == 0).all()
    s, f = R.linear_table(8, 2)             # factor 4: taps 1, 2 and 5, 6 with equal weights
    assert s.tolist() == [1, 5] and f.tolist() == [0.5, 0.5]
    s, f = R.linear_table(7, 7)
    assert s.tolist() == list(range(7)) and (f == 0).all()


def test_shift_clamp_and_crop_of_the_restatement():
    src = R.case_stack(1, (9, 8))[0]
    P = R.prepared(src, (5, 0), 0.0)
    assert np.array_equal(P[:4], np.maximum(src[5:], 0)) and (P[4:] == 0).all()
    P = R.prepared(src, (-2, 3), None)
    assert np.array_equal(P[2:, :5], src[:7, 3:]) and (P[:2] == 0).all() and (P[:, 5:] == 0).all()
    assert (R.prepared(src, (9, 0), -1.0) == 0).all()                       # beyond the image: 0, not lo
    assert np.array_equal(R.prepared(src, (0, 0), None), src)
    nan = src.copy()
    nan[2, 2] = np.nan
    assert np.isnan(R.prepared(nan, (0, 0), 0.0)[2, 2])                     # a NaN stays
    full = R.resize_linear(src, (5, 6), (1, 0), 0.0)
    assert np.array_equal(R.resize_linear(src, (5, 6), (1, 0), 0.0, crop=(1, 2, 3, 4)), full[1:4, 2:6])
    assert np.array_equal(R.resize_area(src[:8], (4, 2), crop=(3, 1, 1, 1)), R.resize_area(src[:8], (4, 2))[3:, 1:])


@pytest.mark.parametrize("shape,factor", R.AREA_CASES + [((70, 1000), (7, 8))], ids=str)
def test_area_against_a_reshape_mean(shape, factor):
    """fy fx - 1 additions and one product, each within u of a partial sum of at most fy fx max|P|: asserted at fy fx u max|P|."""
    fy, fx = factor
    src = R.case_stack(2, shape, seed=2)
    size = (shape[0] // fy, shape[1] // fx)
    got = R.resize_area(src, size, lo=0.0)
    P = R.prepared(src, lo=0.0).astype(np.float64)
    want = P.reshape(2, size[0], fy, size[1], fx).mean(axis=(2, 4))
    err = float(np.abs(got.astype(np.float64) - want).max())
    print("area:", shape, factor, "error %.3g, bound %.3g" % (err, fy * fx * U * P.max()))
    assert got.dtype == np.float32 and got.shape == (2,) + size and err <= fy * fx * U * float(np.abs(P).max())


@pytest.mark.parametrize("k", [3, 5])
@pytest.mark.parametrize("shape", R.MEDIAN_SHAPES, ids=str)
def test_median_equals_scipy(shape, k):
    src = R.case_stack(2, shape, seed=k)
    got = R.median(src, k)
    for v in range(2):
        assert np.array_equal(got[v], ndimage.median_filter(src[v], size=k, mode="nearest"))
    ties = np.round(src * 3)            # many equal values, no negative zero
    ties[ties == 0] = 1.0
    assert np.array_equal(R.median(ties, k)[0], ndimage.median_filter(ties[0], size=k, mode="nearest"))


def test_nan_rules_and_the_conditional_predicate():
    x = np.arange(25, dtype=np.float32).reshape(5, 5)
    x[2, 2] = np.nan
    m = R.median(x, 3)
    # the centre's window holds 6 7 8 11 NaN 13 16 17 18: with the NaN as +inf the rank-4 element is 13
    assert m[2, 2] == 13.0 and np.isfinite(m).all()
    d, rep = R.despeckle(x, 3, np.inf)
    assert rep.sum() == 1 and rep[2, 2] and d[2, 2] == 13.0 and np.array_equal(np.delete(d.ravel(), 12), np.delete(x.ravel(), 12))
    # more than half a window of NaN: the median itself is +inf, and a NaN pixel still takes it
    y = np.full((3, 3), np.nan, dtype=np.float32)
    y[0] = [1.0, 2.0, 3.0]
    m = R.median(y, 3)
    assert m[0, 1] == 3.0 and np.isposinf(m[2, 1])
    d, rep = R.despeckle(y, 3, 1.0)
    assert rep[1:].all() and np.isposinf(d[2]).all() and np.isfinite(d[0]).all()
    # +inf pixels: inf - inf is NaN, so the pixel counts as replaced by a median that is the same +inf
    z = np.full((3, 3), np.inf, dtype=np.float32)
    d, rep = R.despeckle(z, 3, 0.0)
    assert rep.all() and np.isposinf(d).all()
    # an ordinary threshold: one spike on a ramp
    r = np.tile(np.arange(8, dtype=np.float32), (6, 1))
    s = r.copy()
    s[3, 4] = 1e6
    d, rep = R.despeckle(s, 3, 2.0)
    assert rep.sum() == 1 and rep[3, 4] and np.array_equal(d, r)
    # threshold 0 replaces all that differ from their median and nothing else; the result is the median filter
    d, rep = R.despeckle(s, 3, 0.0)
    assert np.array_equal(d, R.median(s, 3)) and np.array_equal(rep, s != R.median(s, 3))
    # k = 5 on a 2 x 2 image: every window is the four pixels with multiplicities 9, 6, 6, 4 (the corner pixel first)
    q = np.array([[1.0, 2.0], [3.0, 4.0]], dtype=np.float32)
    assert np.array_equal(R.median(q, 5), np.array([[2.0, 2.0], [3.0, 3.0]], dtype=np.float32))


# ---- prepare_real.py's host logic -------------------------------------------------------------------------------------------

CONFIG = """[General]
Version=2.5
Comment=FIPS open data set
[Geometry]
DistanceSourceDetector=553.74
DistanceSourceOrigin=210.66
[CT]
NumberImages=12
AngleInterval=30.0
AngleFirst=0.0
AngleLast=330.0
[Detector]
PixelSize=0.050
PixelSizeUnit=mm
"""


def test_config_parser(tmp_path):
    path = tmp_path / "config.txt"
    path.write_text(CONFIG)
    c = PR.parse_config(str(path), 2, 50)
    assert c["n_proj"] == 12 and c["angle_interval"] == 30.0 and c["angle_start"] == 0.0 and c["angle_last"] == 330.0
    assert c["DSD"] == 553.74 / 1000 * 50 and c["DSO"] == 210.66 / 1000 * 50 and c["dDetector"] == 0.050 * 2 / 1000 * 50
    angles = PR.scan_angles(c)
    assert angles.shape == (12,) and np.array_equal(angles, np.concatenate([np.arange(0.0, 330.0, 30.0), [330.0]]) / 180.0 * np.pi)
    path.write_text(CONFIG.replace("PixelSize=0.050\n", ""))      # PixelSizeUnit alone is no pixel size
    with pytest.raises(ValueError, match="PixelSize"):
        PR.parse_config(str(path), 2, 50)


@pytest.mark.parametrize("n_proj,n_train,n_test", [(12, 4, 3), (721, 75, 100), (361, 50, 100)])
def test_id_selection_is_the_references(n_proj, n_train, n_test):
    state = random.getstate()
    try:
        random.seed(0)
        train_ids = np.linspace(0, n_proj - 1, n_train).astype(int)
        test_ids = sorted(random.sample(np.setdiff1d(np.arange(n_proj), train_ids).tolist(), n_test))
    finally:
        random.setstate(state)
    before = random.getstate()
    got_train, got_test = PR.select_ids(n_proj, n_train, n_test)
    assert np.array_equal(got_train, train_ids) and got_test == test_ids and len(set(got_test) & set(train_ids.tolist())) == 0
    assert random.getstate() == before            # the caller's generator is left alone


def test_crop_rule():
    for mh, mw in [(20, 24), (24, 20), (560, 592), (27, 24), (24, 29), (5, 5), (2, 6)]:
        assert PR.crop_window(mh, mw) == R.square_window(mh, mw), (mh, mw)
    assert PR.crop_window(560, 592) == (0, 16, 560, 560) and PR.crop_window(27, 24) == (1, 0, 25, 24)
    for mh, mw in [(20, 21), (21, 20), (1, 2)]:
        assert R.square_window(mh, mw) is None            # the reference's [0:-0] slice is empty
        with pytest.raises(ValueError, match="differ by one"):
            PR.crop_window(mh, mw)
    assert PR.resized_size(2240, 2368, 4) == (560, 592) and PR.resized_size(41, 47, 2) == (20, 23)


def test_parser_defaults_are_the_references():
    a = PR.parser().parse_args(["--data", "in", "--output", "out"])
    assert (a.proj_subsample, a.proj_rescale, a.object_scale, a.n_test, a.n_train) == (4, 400.0, 50, 100, 75)
    assert a.nVoxel == [256, 256, 256] and a.sVoxel == [2.0, 2.0, 2.0] and a.offOrigin == [0.0, 0.0, 0.0]
    assert a.offDetector == [0.0, 0.0] and a.accuracy == 0.5
    assert a.interpolation == "linear" and a.despeckle is None and a.despeckle_size == 3


# ---- refusals ------------------------------------------------------------------------------------------------------------------

def test_host_tensors_and_bad_arguments_are_refused():
    x = torch.rand(2, 8, 12)
    for fn, args in ((PJ.resize, (x, (4, 6))), (PJ.resize, (x.numpy(), (4, 6))), (PJ.resize, (x, (4, 6), "area")),
                     (PJ.median_filter, (x,)), (PJ.median_filter, (x.numpy(), 5)), (PJ.despeckle, (x, 1.0)),
                     (PJ.despeckle, (x[0], 1.0, 5, True)), (PJ.normalize, (x, x[0])), (PJ.normalize, (x, x[0].numpy()))):
        with pytest.raises(R2HipError):
            fn(*args)
    # arguments that do not depend on the projections are checked first: no tensor is touched, nothing is launched
    for fn, args, kw in ((PJ.resize, (x, (0, 6)), {}), (PJ.resize, (x, (4,)), {}), (PJ.resize, (x, 4), {}), (PJ.resize, (x, (4.5, 6)), {}),
                         (PJ.resize, (x, (4, 6)), {"interpolation": "cubic"}), (PJ.resize, (x, (4, 6)), {"shift": (1,)}),
                         (PJ.resize, (x, (4, 6)), {"shift": (0.5, 0)}), (PJ.resize, (x, (4, 6)), {"lo": float("nan")}),
                         (PJ.resize, (x, (4, 6)), {"crop": (0, 0, 5, 6)}), (PJ.resize, (x, (4, 6)), {"crop": (3, 0, 2, 6)}),
                         (PJ.resize, (x, (4, 6)), {"crop": (0, 0, 0, 6)}), (PJ.resize, (x, (4, 6)), {"crop": (-1, 0, 2, 2)}),
                         (PJ.resize, (x, (4, 6)), {"crop": (0, 0, 4)}), (PJ.resize, (x, (2 ** 16, 2 ** 15)), {}),
                         (PJ.median_filter, (x, 4), {}), (PJ.median_filter, (x, 7), {}), (PJ.median_filter, (x, True), {}),
                         (PJ.despeckle, (x, -1.0), {}), (PJ.despeckle, (x, float("nan")), {}), (PJ.despeckle, (x, 1.0, 2), {})):
        with pytest.raises(ValueError):
            fn(*args, **kw)


def test_the_library_refuses_before_any_launch():
    """R2_ERR_INVALID comes back before the first launch, so these calls need no GPU: the pointers are never followed."""
    L = _lib.lib()
    p, ws = 4096, 1 << 20                  # stand-ins for device pointers
    ok = dict(V=2, H=8, W=12, src=p, sr=0, sc=0, lo=0.0, interp=0, mh=4, mw=6, r0=0, c0=0, oh=4, ow=6, dst=p, ws=p, ws_bytes=ws)
    bad = [dict(V=-1), dict(H=0), dict(W=-3), dict(mh=0), dict(mw=0), dict(interp=2), dict(interp=-1), dict(oh=0), dict(ow=0),
           dict(r0=-1), dict(c0=-1), dict(r0=1), dict(c0=1), dict(oh=5), dict(ow=7), dict(lo=float("nan")), dict(sr=2 ** 30 + 1),
           dict(sc=-2 ** 30 - 1), dict(src=None), dict(dst=None), dict(ws=None), dict(ws_bytes=(4 + 6) * 8 - 1),
           dict(interp=1, mh=3, oh=3), dict(interp=1, mw=5, ow=5),                       # area with a factor that is no integer
           dict(H=2 ** 16, W=2 ** 15), dict(mh=2 ** 16, mw=2 ** 15, oh=1, ow=1), dict(V=2 ** 31 - 1, H=2 ** 10, W=2 ** 10)]
    for change in bad:
        a = dict(ok, **change)
        rc = L.r2_proj_resize(*[a[k] for k in ("V", "H", "W", "src", "sr", "sc", "lo", "interp", "mh", "mw", "r0", "c0", "oh",
                                               "ow", "dst", "ws", "ws_bytes")], None)
        assert rc == _lib.R2_ERR_INVALID, change
        assert L.r2_last_error()
    assert L.r2_proj_resize_workspace_bytes(4, 6) == 80 and L.r2_proj_resize_workspace_bytes(0, 6) == 0
    okm = dict(V=2, H=8, W=12, src=p, k=3, conditional=1, threshold=1.0, dst=p, flagged=None)
    badm = [dict(V=-1), dict(H=0), dict(W=0), dict(k=4), dict(k=1), dict(k=7), dict(conditional=2), dict(conditional=-1),
            dict(threshold=float("nan")), dict(src=None), dict(dst=None), dict(H=2 ** 16, W=2 ** 15),
            dict(V=2 ** 31 - 1, H=2 ** 10, W=2 ** 10),
            dict(V=2 ** 30, H=17, W=1)]                                     # 2^31 tiles of 64 x 16
    for change in badm:
        a = dict(okm, **change)
        rc = L.r2_proj_median(*[a[k] for k in ("V", "H", "W", "src", "k", "conditional", "threshold", "dst", "flagged")], None)
        assert rc == _lib.R2_ERR_INVALID, change
    # V = 0 is a no-op, whatever the pointers
    assert L.r2_proj_resize(0, 8, 12, None, 0, 0, 0.0, 0, 4, 6, 0, 0, 4, 6, None, None, 0, None) == 0
    assert L.r2_proj_median(0, 8, 12, None, 3, 0, 0.0, None, None, None) == 0
