"""Conditioning of measured projections on the MI355X (csrc/projections.hip, r2_gaussian_amd/projections.py, prepare_real.py):
the resize and the median bit for bit against the float32 restatement (tests/projections_ref.py, which
tests/test_projections_cpu.py pins to torch and scipy), the Python surface, validation before any launch, and the real-data
driver end to end."""
import json
import os

import numpy as np
import pytest
import scipy.io
import scipy.ndimage as ndimage
import torch

from r2_gaussian_amd import _lib
from r2_gaussian_amd import fdk as F
from r2_gaussian_amd import prepare_real as PR
from r2_gaussian_amd import projections as PJ
from r2_gaussian_amd import recon
from r2_gaussian_amd._boundary import call
from r2_gaussian_amd._lib import R2HipError
from tests import projections_ref as R

pytestmark = pytest.mark.gpu

# The kernels' constants (csrc/projections.hip).  The resize takes TB = 256 outputs per workgroup, numbered over (view, row,
# column) of the cropped result: the edge shapes below give rows of 255, 256 and 257 outputs and whole results (V = 1) of 255,
# 256 and 257.  The median's workgroup owns a tile of MED_TX x MED_TY = 64 x 16 pixels and stages a halo of k / 2 around it:
# (16, 64) is one tile exactly, (16, 65) and (17, 64) one column and one row more, (15, 63) one less each way; (1, 130) and
# (67, 1) are lines across three and five tiles, and (2, 2) with k = 5 has a halo that exceeds the image on both sides.
RESIZE_EDGE_SHAPES = [((4, 300), (2, 255)), ((4, 300), (2, 256)), ((4, 300), (2, 257)), ((20, 40), (15, 17)), ((20, 40), (16, 16)),
                      ((300, 2), (257, 1))]
MEDIAN_SHAPES = [(1, 1), (2, 2), (1, 130), (67, 1), (16, 64), (16, 65), (17, 64), (15, 63), (33, 70)]


def _bits_equal(got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    return got.dtype == want.dtype == np.float32 and got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32))


def _crops(size):
    """The full image, the far corner, and where there is room a window strictly inside."""
    mh, mw = size
    out = [None, (mh // 2, mw // 2, mh - mh // 2, mw - mw // 2)]
    if mh >= 3 and mw >= 3:
        out.append((1, 1, mh - 2, mw - 2))
    return out


@pytest.mark.parametrize("V", [1, 3])
@pytest.mark.parametrize("shape,size", R.RESIZE_SHAPES + RESIZE_EDGE_SHAPES, ids=lambda v: "x".join(map(str, v)))
def test_linear_resize_equals_the_float32_restatement_bit_for_bit(gpu, shape, size, V):
    src = R.case_stack(V, shape)
    assert (src < 0).any() or src.size < 4
    t = torch.from_numpy(src).to(gpu)
    H = shape[0]
    for shift in ((5, 0), (-2, 3), (H, 0), (0, 0)):
        for lo in (0.0, None):
            for crop in _crops(size):
                want = R.resize_linear(src, size, shift, lo, crop)
                got = PJ.resize(t, size, "linear", shift, lo, crop).cpu().numpy()
                assert _bits_equal(got, want), (shift, lo, crop, float(np.abs(got.astype(np.float64) - want).max()))
                if shift == (H, 0):
                    assert not got.any()                       # everything moved out: zeros, not lo
                if lo == 0.0:
                    assert float(got.min()) >= 0.0
    assert np.array_equal(t.cpu().numpy(), src)                # the input is untouched


@pytest.mark.parametrize("shape,factor", R.AREA_CASES, ids=str)
def test_area_resize_equals_the_float32_restatement_bit_for_bit(gpu, shape, factor):
    size = (shape[0] // factor[0], shape[1] // factor[1])
    for V in (1, 3):
        src = R.case_stack(V, shape, seed=2)
        t = torch.from_numpy(src).to(gpu)
        for shift, lo in (((0, 0), None), ((1, 0), 0.0), ((-1, 2), 0.0), ((shape[0], 0), -1.0)):
            for crop in _crops(size):
                want = R.resize_area(src, size, shift, lo, crop)
                got = PJ.resize(t, size, "area", shift, lo, crop).cpu().numpy()
                assert _bits_equal(got, want), (V, shift, lo, crop)
        assert np.array_equal(t.cpu().numpy(), src)


def test_resize_surface(gpu):
    shape, size = (37, 300), (9, 70)
    src = R.case_stack(3, shape)
    t = torch.from_numpy(src).to(gpu)
    want = R.resize_linear(src, size, (5, 0), 0.0, (1, 2, 7, 60))
    a = PJ.resize(t, size, shift=(5, 0), lo=0.0, crop=(1, 2, 7, 60))
    assert _bits_equal(a.cpu().numpy(), want)
    assert torch.equal(PJ.resize(t, size, shift=(5, 0), lo=0.0, crop=(1, 2, 7, 60)), a)                      # two runs
    out = torch.full((3, 7, 60), float("nan"), device=gpu)
    assert PJ.resize(t, size, shift=(5, 0), lo=0.0, crop=(1, 2, 7, 60), out=out) is out and torch.equal(out, a)   # out= is honoured
    # one projection [H,W]; other dtypes and layouts are converted
    one = PJ.resize(t[1], size, shift=(5, 0), lo=0.0, crop=(1, 2, 7, 60))
    assert one.shape == (7, 60) and torch.equal(one, a[1])
    assert torch.equal(PJ.resize(t.double(), size, shift=(5, 0), lo=0.0, crop=(1, 2, 7, 60)), a)
    tt = t.permute(0, 2, 1)
    assert torch.equal(PJ.resize(tt, (70, 9)), PJ.resize(tt.contiguous(), (70, 9)))
    # a NaN-filled, oversized workspace through the C ABI; V = 0 writes nothing
    nbytes = int(_lib.lib().r2_proj_resize_workspace_bytes(*size))
    assert nbytes == (9 + 70) * 8
    ws = torch.full((nbytes // 4 + 100,), float("nan"), device=gpu)
    out.fill_(float("nan"))
    call("r2_proj_resize", gpu, 3, 37, 300, t, 5, 0, 0.0, 0, 9, 70, 1, 2, 7, 60, out, ws, ws.numel() * 4)
    assert torch.equal(out, a)
    out.fill_(7.0)
    call("r2_proj_resize", gpu, 0, 37, 300, t, 5, 0, 0.0, 0, 9, 70, 1, 2, 7, 60, out, ws, ws.numel() * 4)
    call("r2_proj_median", gpu, 0, 7, 60, t, 3, 1, 1.0, out, None)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    # area without a workspace
    b = torch.empty((3, 37, 100), device=gpu)
    call("r2_proj_resize", gpu, 3, 37, 300, t, 0, 0, float("-inf"), 1, 37, 100, 0, 0, 37, 100, b, None, 0)
    assert _bits_equal(b.cpu().numpy(), R.resize_area(src, (37, 100)))
    # normalize: -log of the transmission
    raw = torch.rand(2, 5, 6, device=gpu) * 900 + 100
    flat, dark = torch.full((5, 6), 1100.0, device=gpu), torch.full((5, 6), 50.0, device=gpu)
    assert torch.allclose(PJ.normalize(raw, flat, dark), -torch.log((raw - 50.0) / 1050.0))
    assert torch.isfinite(PJ.normalize(torch.zeros(5, 6, device=gpu), flat)).all()


def _median_stack(shape, with_specials):
    """Three distinct views; with specials a NaN, a +inf and a -inf pixel on their own and a block of NaN that fills more than
    half of a 5 x 5 window (where the image has the room)."""
    src = R.case_stack(3, shape, seed=5)
    if with_specials:
        H, W = shape
        flat = src.reshape(3, -1)
        n = flat.shape[1]
        flat[0, n // 2] = np.nan
        if n >= 8:
            flat[1, n // 3] = np.inf
            flat[1, n - 1] = -np.inf
            flat[2, 0] = np.nan
        if H >= 6 and W >= 6:
            src[2, 1:5, 2:6] = np.nan
            src[0, H - 3:, W - 3:] = np.nan
        elif n >= 40:
            (src[2, 0, 10:30] if H == 1 else src[2, 10:30, 0])[...] = np.nan
    return src


@pytest.mark.parametrize("k", [3, 5])
@pytest.mark.parametrize("shape", MEDIAN_SHAPES, ids=lambda s: "%dx%d" % s)
def test_median_and_despeckle_equal_the_restatement_bit_for_bit(gpu, shape, k):
    for with_specials in (False, True):
        src = _median_stack(shape, with_specials)
        t = torch.from_numpy(src).to(gpu)
        want_m = R.median(src, k)
        got_m = PJ.median_filter(t, k).cpu().numpy()
        assert _bits_equal(got_m, want_m), with_specials
        if not with_specials:
            for v in range(3):
                assert np.array_equal(got_m[v], ndimage.median_filter(src[v], size=k, mode="nearest"))
        for threshold in (0.0, float("inf"), 0.6):
            want, want_rep = R.despeckle(src, k, threshold)
            got, mask = PJ.despeckle(t, threshold, k, return_mask=True)
            got, mask = got.cpu().numpy(), mask.cpu().numpy()
            assert mask.dtype == np.bool_ and np.array_equal(mask, want_rep), threshold
            assert _bits_equal(got, want), threshold
            assert not np.isnan(got).any()                                           # every NaN pixel is replaced
            changed = ~((got == src) | (np.isnan(got) & np.isnan(src)))
            assert np.array_equal(changed, mask & ~(want_m == src))                  # the mask is what changed
            if threshold == float("inf"):
                assert np.array_equal(mask, np.isnan(src) | (np.isinf(src) & (src == want_m)))   # inf - inf
            assert torch.equal(PJ.despeckle(t, threshold, k), torch.from_numpy(got).to(gpu))   # without the mask; two runs
        assert np.array_equal(t.cpu().numpy(), src, equal_nan=True)                  # the input is untouched
    one = PJ.median_filter(t[1], k)                                                  # one projection [H,W]
    assert one.shape == shape and _bits_equal(one.cpu().numpy(), want_m[1])


def test_median_through_the_c_abi(gpu):
    src = _median_stack((17, 64), True)
    t = torch.from_numpy(src).to(gpu)
    dst = torch.full((3, 17, 64), float("nan"), device=gpu)
    flagged = torch.full((3, 17, 64), 9, dtype=torch.uint8, device=gpu)
    call("r2_proj_median", gpu, 3, 17, 64, t, 5, 0, 0.6, dst, flagged)               # conditional = 0: the median, and the mask
    assert _bits_equal(dst.cpu().numpy(), R.median(src, 5))
    assert np.array_equal(flagged.cpu().numpy().astype(bool), R.despeckle(src, 5, 0.6)[1])
    assert int(flagged.max()) <= 1


def test_no_host_sync(gpu):
    t = torch.from_numpy(R.case_stack(3, (37, 300))).to(gpu)
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        a = PJ.resize(t, (9, 70), shift=(5, 0), lo=0.0, crop=(0, 5, 9, 60))
        b = PJ.resize(t, (37, 100), "area")
        c = PJ.median_filter(t, 5)
        d, m = PJ.despeckle(t, 0.5, return_mask=True)
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    assert a.shape == (3, 9, 60) and b.shape == (3, 37, 100) and c.shape == t.shape and d.shape == m.shape == t.shape


def test_validation_before_any_launch(gpu):
    t = torch.rand(2, 8, 12, device=gpu)
    out = torch.full((2, 4, 6), 7.0, device=gpu)
    nbytes = int(_lib.lib().r2_proj_resize_workspace_bytes(4, 6))
    ws = torch.full((nbytes // 4,), 7.0, device=gpu)
    flagged = torch.full((2, 8, 12), 7, dtype=torch.uint8, device=gpu)
    full = torch.full((2, 8, 12), 7.0, device=gpu)
    ok = (2, 8, 12, t, 0, 0, 0.0, 0, 4, 6, 0, 0, 4, 6, out, ws, nbytes)
    bad = []
    for i, v in ((0, -1), (1, 0), (2, 0), (3, None), (7, 2), (8, 0), (9, 0), (10, 1), (11, -1), (12, 5), (13, 0), (14, None), (15, None),
                 (16, nbytes - 1), (6, float("nan")), (4, 2 ** 30 + 1)):
        a = list(ok)
        a[i] = v
        bad.append(("r2_proj_resize", tuple(a)))
    bad.append(("r2_proj_resize", (2, 8, 12, t, 0, 0, 0.0, 1, 3, 6, 0, 0, 3, 6, out, ws, nbytes)))       # area, 8 / 3
    bad.append(("r2_proj_resize", (2, 8, 12, t, 0, 0, 0.0, 1, 4, 5, 0, 0, 4, 5, out, ws, nbytes)))       # area, 12 / 5
    okm = (2, 8, 12, t, 3, 1, 1.0, full, flagged)
    for i, v in ((0, -1), (1, 0), (2, -1), (3, None), (4, 4), (4, 9), (5, 2), (6, float("nan")), (7, None)):
        a = list(okm)
        a[i] = v
        bad.append(("r2_proj_median", tuple(a)))
    for name, args in bad:
        with pytest.raises(R2HipError):
            call(name, gpu, *args)
    # the Python surface
    for fn, args, kw in ((PJ.resize, (t, (3, 6), "area"), {}), (PJ.resize, (t, (4, 5), "area"), {}), (PJ.resize, (t, (4, 6), "nearest"), {}),
                         (PJ.resize, (t, (0, 6)), {}), (PJ.resize, (t, (4, 6)), {"crop": (1, 0, 4, 6)}),
                         (PJ.resize, (t, (4, 6)), {"out": torch.empty(2, 4, 7, device=gpu)}),
                         (PJ.resize, (t, (4, 6)), {"out": out.double()}), (PJ.resize, (t[0, 0], (4, 6)), {}),
                         (PJ.resize, (t[None], (4, 6)), {}), (PJ.resize, (t[:, :0], (4, 6)), {}),
                         (PJ.median_filter, (t, 4), {}), (PJ.median_filter, (t[0, 0],), {}), (PJ.despeckle, (t, -1.0), {}),
                         (PJ.despeckle, (t, 1.0, 7), {})):
        with pytest.raises(ValueError):
            fn(*args, **kw)
    for fn, args, kw in ((PJ.resize, (t.cpu(), (4, 6)), {}), (PJ.resize, (t, (4, 6)), {"out": out.cpu()}),
                         (PJ.median_filter, (t.cpu().numpy(),), {}), (PJ.despeckle, (t.cpu(), 1.0), {})):
        with pytest.raises(R2HipError):
            fn(*args, **kw)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((ws == 7.0).all()) and bool((flagged == 7).all()) and bool((full == 7.0).all())


# ---- the driver, end to end ----------------------------------------------------------------------------------------------------

CONFIG = """[Geometry]
DistanceSourceDetector=553.74
DistanceSourceOrigin=210.66
[CT]
NumberImages=12
AngleInterval=30.0
AngleFirst=0.0
AngleLast=330.0
[Detector]
PixelSize=0.8
PixelSizeUnit=mm
"""
DRIVER_ARGS = ["--proj_subsample", "2", "--n_train", "4", "--n_test", "3", "--nVoxel", "16", "16", "16"]


def _write_scan(folder, images):
    os.makedirs(folder)
    with open(os.path.join(folder, "config.txt"), "w") as f:
        f.write(CONFIG)
    for i, img in enumerate(images):
        scipy.io.savemat(os.path.join(folder, "scan_%03d.mat" % i), {"img": img})


def _scan_images():
    """12 measured projections of 40 x 48 in detector units: a bright disc on a noisy background, a fifth of it negative."""
    rng = np.random.RandomState(11)
    yy, xx = np.mgrid[:40, :48]
    disc = 24.0 * np.sqrt(np.maximum(0.0, 1.0 - ((yy - 22) / 13.0) ** 2 - ((xx - 24) / 15.0) ** 2))
    return [disc * (1.0 + 0.05 * np.cos(i)) + rng.randn(40, 48) * 1.5 + 1.0 for i in range(12)]


def test_driver_end_to_end(gpu, tmp_path):
    images = _scan_images()
    _write_scan(str(tmp_path / "scan"), images)
    case = str(tmp_path / "case")
    meta = PR.main(["--data", str(tmp_path / "scan"), "--output", case] + DRIVER_ARGS)
    with open(os.path.join(case, "meta_data.json")) as f:
        saved = json.load(f)
    assert saved == json.loads(json.dumps(meta))

    # the projections: the restatement of the steps, 20 x 20, nothing negative, the five-row shift visible
    assert (np.concatenate([R.host_scale(im, 400.0, 50) for im in images]) < 0).any()
    for i, img in enumerate(images):
        got = np.load(os.path.join(case, "proj_all", "scan_%03d.npy" % i))
        want = R.real_projection(img, 400.0, 50, 2)
        assert got.shape == (20, 20) and _bits_equal(got, want), i
        assert float(got.min()) >= 0.0
        # 40 rows moved up by 5 leave rows 35 .. 39 empty: output rows 18 and 19 read rows 36 .. 39, row 17 reads 34 and 35
        assert not got[18:].any() and got[17].any()
        unshifted = R.resize_linear(R.host_scale(img, 400.0, 50), (20, 24), (0, 0), 0.0, (0, 2, 20, 20))
        rows = np.arange(20, dtype=np.float64)[:, None]
        moved = float((rows * unshifted).sum() / unshifted.sum() - (rows * got).sum() / got.sum())
        assert 2.0 < moved < 3.0, moved                        # the disc sits 5 / 2 output rows higher

    # the splits: the reference's statements
    import random
    state = random.getstate()
    random.seed(0)
    train_ids = np.linspace(0, 12 - 1, 4).astype(int)
    test_ids = sorted(random.sample(np.setdiff1d(np.arange(12), train_ids).tolist(), 3))
    random.setstate(state)
    angles = np.concatenate([np.arange(0.0, 330.0, 30.0), [330.0]]) / 180.0 * np.pi
    for split, ids in (("proj_train", train_ids), ("proj_test", test_ids)):
        assert [e["file_path"] for e in saved[split]] == [os.path.join(split, "scan_%03d.npy" % i) for i in ids]
        assert [e["angle"] for e in saved[split]] == [float(angles[i]) for i in ids]
        assert sorted(os.listdir(os.path.join(case, split))) == ["scan_%03d.npy" % i for i in ids]
        for i in ids:
            assert np.array_equal(np.load(os.path.join(case, split, "scan_%03d.npy" % i)),
                                  np.load(os.path.join(case, "proj_all", "scan_%03d.npy" % i)))

    # the meta-data: the reference's scanner block, "ct" and "vol"
    d = 0.8 * 2 / 1000 * 50
    assert saved["scanner"] == {"mode": "cone", "DSD": 553.74 / 1000 * 50, "DSO": 210.66 / 1000 * 50, "nDetector": [20, 20],
                                "sDetector": [20 * d, 20 * d], "nVoxel": [16, 16, 16], "sVoxel": [2.0, 2.0, 2.0],
                                "offOrigin": [0.0, 0.0, 0.0], "offDetector": [0.0, 0.0], "accuracy": 0.5, "totalAngle": 330.0,
                                "startAngle": 0.0, "noise": True, "filter": None}
    assert saved["vol"] == "vol_gt.npy" and saved["ct"] == "vol_gt.npy" and saved["radius"] == 1.0
    assert saved["bbox"] == [[-1.0, -1.0, -1.0], [1.0, 1.0, 1.0]]

    # the ground truth: FDK of proj_all, clamped at 0; kept when it exists
    stack = np.stack([np.load(os.path.join(case, "proj_all", "scan_%03d.npy" % i)) for i in range(12)])
    want_vol = F.fdk(stack, angles, saved["scanner"]).clamp_min(0.0).cpu().numpy()
    vol = np.load(os.path.join(case, "vol_gt.npy"))
    assert vol.shape == (16, 16, 16) and vol.dtype == np.float32 and np.array_equal(vol, want_vol) and vol.max() > 0 and vol.min() == 0
    np.save(os.path.join(case, "vol_gt.npy"), np.full((16, 16, 16), 3.0, dtype=np.float32))
    PR.main(["--data", str(tmp_path / "scan"), "--output", case] + DRIVER_ARGS)
    assert (np.load(os.path.join(case, "vol_gt.npy")) == 3.0).all()
    np.save(os.path.join(case, "vol_gt.npy"), vol)

    # the round trip through the readers
    c = recon._read_case(case)
    assert c["vol"].shape == (16, 16, 16) and c["train"][0].shape == (4, 20, 20) and c["test"][0].shape == (3, 20, 20)
    assert np.array_equal(c["train"][1], angles[train_ids]) and c["cfg"] == saved["scanner"] and c["weights_train"] is None

    # --despeckle: a spike and a NaN planted in one projection are removed, everything else is the run without the flag
    spoiled = [im.copy() for im in images]
    spoiled[6][20, 30] = 1e6 * 400.0 / 50          # 1e6 after the host's scaling
    spoiled[6][11, 9] = np.nan
    _write_scan(str(tmp_path / "scan_spoiled"), spoiled)
    case2 = str(tmp_path / "case_despeckled")
    PR.main(["--data", str(tmp_path / "scan_spoiled"), "--output", case2, "--despeckle", "100"] + DRIVER_ARGS)
    dirty = R.real_projection(spoiled[6], 400.0, 50, 2)
    clean = R.real_projection(images[6], 400.0, 50, 2)
    touched = ~(dirty == clean)
    assert touched.sum() == 2 and np.isnan(dirty).sum() == 1 and np.nanmax(dirty) > 1e5
    for i in range(12):
        got = np.load(os.path.join(case2, "proj_all", "scan_%03d.npy" % i))
        first = np.load(os.path.join(case, "proj_all", "scan_%03d.npy" % i))
        if i != 6:
            assert _bits_equal(got, first), i
            continue
        assert _bits_equal(got, R.real_projection(spoiled[6], 400.0, 50, 2, despeckle_threshold=100.0))
        assert np.array_equal(got[~touched], first[~touched]) and np.isfinite(got).all() and float(got.max()) < 10.0
        assert np.abs(got[touched] - first[touched]).max() < 1.0          # the two pixels took their neighbourhood's median
    assert np.isfinite(np.load(os.path.join(case2, "vol_gt.npy"))).all()


def test_driver_options(gpu, tmp_path):
    images = _scan_images()[:3]
    host = np.stack([R.host_scale(im, 400.0, 50) for im in images])
    t = torch.from_numpy(host).to(gpu)
    # the box mean, and --proj_subsample 1: clamp and shift alone
    got = PR.condition(t, 2, "area").cpu().numpy()
    assert _bits_equal(got, R.resize_area(host, (20, 24), (5, 0), 0.0, (0, 2, 20, 20)))
    got = PR.condition(t, 1).cpu().numpy()
    assert _bits_equal(got, R.prepared(host, (5, 0), 0.0))
    got = PR.condition(t, 2, "linear", 0.5, 5).cpu().numpy()
    assert _bits_equal(got, R.resize_linear(R.despeckle(host, 5, 0.5)[0], (20, 24), (5, 0), 0.0, (0, 2, 20, 20)))
    # 42 x 48 at a factor of 2 is 21 x 24, cropped to 21 x 22 as the reference's slice leaves it; 44 columns give 21 x 22: refused
    assert PR.condition(torch.zeros(1, 42, 48, device=gpu), 2).shape == (1, 21, 22)
    with pytest.raises(ValueError, match="differ by one"):
        PR.condition(torch.zeros(1, 42, 44, device=gpu), 2)
    # .npy projections are read when there is no .mat
    folder = tmp_path / "scan_npy"
    os.makedirs(str(folder))
    (folder / "config.txt").write_text(CONFIG.replace("NumberImages=12", "NumberImages=3").replace("AngleLast=330.0", "AngleLast=60.0"))
    for i, im in enumerate(images):
        np.save(str(folder / ("p%d.npy" % i)), im)
    case = str(tmp_path / "case_npy")
    PR.main(["--data", str(folder), "--output", case, "--proj_subsample", "2", "--n_train", "2", "--n_test", "1", "--nVoxel", "8", "8",
             "8", "--batch", "2", "--interpolation", "area"])
    got = np.load(os.path.join(case, "proj_all", "p1.npy"))
    assert _bits_equal(got, R.resize_area(host[1], (20, 24), (5, 0), 0.0, (0, 2, 20, 20)))
    assert recon._read_case(case)["train"][0].shape == (2, 20, 20)
