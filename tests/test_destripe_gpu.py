"""Stripe removal on the MI355X (csrc/destripe.hip, r2_gaussian_amd/projections.py: destripe, stripe_offsets; prepare_real.py's
--destripe) against the NumPy / SciPy restatement (tests/destripe_ref.py, which tests/test_destripe_cpu.py pins): equal bit
for bit, numerically where a -0 and a +0 can tie; the stable order on stacks full of ties; the NaN rules; the Python surface;
validation before any launch; and the converter end to end."""
import io
import json
import os

import numpy as np
import pytest
import torch

from r2_gaussian_amd import _lib
from r2_gaussian_amd import prepare_real as PR
from r2_gaussian_amd import projections as PJ
from r2_gaussian_amd import recon
from r2_gaussian_amd._boundary import call
from r2_gaussian_amd._lib import R2HipError
from tests import destripe_ref as R
from tests import projections_ref as PREF

pytestmark = pytest.mark.gpu

# The kernels' constants (csrc/destripe.hip).  The two transposes move tiles of TR x TR = 64 x 64 (views x pixels): 63, 64 and 65
# views, and H W of 63, 64, 65 pixels, sit on either side of a tile.  The sort pads a column to N keys, the power of two that
# holds V, so 2^n - 1, 2^n and 2^n + 1 views are the last one and two sizes of one network and the first of the next; below
# SORT_ITEMS = 512 keys a workgroup sorts 512 / N columns at once, and H W = 3, 5, 15 ... leave its last group short.  V = 4096 is
# R2_DESTRIPE_MAX_VIEWS.  The median's workgroup owns MED_TW = 32 columns (8 per lane) and MED_RC = 64 ranks and stages a halo of
# k / 2 columns: W = 31, 32, 33 and 63, 64, 65 are the strips' edges, W < k and W <= k / 2 make the halo wider than the row.
# The mean method's subtraction takes SUB_VIEWS = 8 views per lane: 1, 2 and 63 .. 65 views cover a short and a full chunk.
VIEWS = [1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 100, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025]
VIEWS_LONG = [2047, 2048, 2049, 4095, 4096]                      # at H = 1, W = 3
WIDTHS = [1, 2, 15, 31, 32, 33, 63, 64, 65, 130]
SIZES = [3, 9, 31]


def _bits_equal(got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    return got.dtype == want.dtype == np.float32 and got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32))


def _bits_equal_nan_for_nan(got, want):
    """Bit for bit, but a NaN for a NaN whatever its sign and payload, which the header does not state."""
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and _bits_equal(np.where(nan, np.float32(0), got), np.where(nan, np.float32(0), want))


def _both_equal_the_restatement(gpu, src, k, bitwise=True):
    t = torch.from_numpy(src).to(gpu)
    equal = _bits_equal if bitwise else (lambda a, b: a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True))
    got = PJ.destripe(t, k, "sort").cpu().numpy()
    assert equal(got, R.destripe_sort(src, k)), ("sort", src.shape, k)
    got, off = PJ.destripe(t, k, "mean", return_offsets=True)
    want, want_off = R.destripe_mean(src, k)
    assert _bits_equal_nan_for_nan(got.cpu().numpy(), want) and _bits_equal_nan_for_nan(off.cpu().numpy(), want_off), ("mean", src.shape, k)
    assert np.array_equal(t.cpu().numpy(), src, equal_nan=True)                      # the input is untouched


@pytest.mark.parametrize("V", VIEWS)
def test_every_view_count_equals_the_restatement_bit_for_bit(gpu, V):
    for H, W, k in ((3, 5, 3), (1, 21, 9)):
        _both_equal_the_restatement(gpu, R.case_stack(V, H, W), k)


@pytest.mark.parametrize("V", VIEWS_LONG)
def test_the_longest_columns_equal_the_restatement_bit_for_bit(gpu, V):
    for k in (3, 31):                                                                # k / 2 >= W
        _both_equal_the_restatement(gpu, R.case_stack(V, 1, 3), k)


@pytest.mark.parametrize("H", [1, 3])
@pytest.mark.parametrize("W", WIDTHS)
def test_every_width_and_window_equals_the_restatement_bit_for_bit(gpu, W, H):
    src = R.case_stack(70, H, W)
    for k in SIZES:
        _both_equal_the_restatement(gpu, src, k)


def test_ties_keep_the_order_of_the_views(gpu):
    """More than half zeros, eight levels, one level: an unstable sort puts the tied views' values back in another order."""
    x = R.case_stack(257, 3, 70, seed=1)
    clamped = np.maximum(x - np.float32(0.3), np.float32(0))
    assert (clamped == 0).mean() > 0.5
    clamped[5:40, 1, 10:20] = np.float32(-0.0)                                       # -0 ties with +0
    levels = (np.clip(np.floor(x * 4.0), -4, 3) / 4.0).astype(np.float32)
    assert len(np.unique(levels)) <= 8
    for src in (clamped, levels, np.full((65, 2, 33), 0.5, np.float32)):
        for k in (3, 9):
            _both_equal_the_restatement(gpu, src, k, bitwise=False)
    flat = np.full((65, 2, 33), 0.5, np.float32)
    assert _bits_equal(PJ.destripe(torch.from_numpy(flat).to(gpu), 9).cpu().numpy(), flat)


def test_nan_rules(gpu):
    src = R.case_stack(65, 3, 40, seed=2)
    src[7, 0, 3] = np.nan
    src[[1, 30, 64], 1, 20] = np.nan
    src[:, 2, 11] = np.nan                                                           # a pixel that never measured
    src[:, 2, 30:36] = np.nan                                                        # more than half of a window of 9
    src[3, 0, 39] = np.inf
    src[4, 0, 0] = -np.inf
    for k in (1, 3, 9):                                                              # k = 1: the one-pass copy
        _both_equal_the_restatement(gpu, src, k, bitwise=False)
    t = torch.from_numpy(src).to(gpu)
    got = PJ.destripe(t, 9, "sort").cpu().numpy()
    # a NaN is read as +inf: a lone dead pixel takes its neighbours' values, the middle of six dead columns stays +inf
    assert not np.isnan(got).any() and np.isfinite(got[:, 2, 11]).all() and np.isinf(got[:, 2, 32]).all()
    got, off = PJ.destripe(t, 9, "mean", return_offsets=True)
    got, off = got.cpu().numpy(), off.cpu().numpy()
    nan_pixels = np.isnan(src).any(axis=0) | np.isinf(src).any(axis=0)               # +-inf: a mean of inf, inf - inf in d
    assert np.isnan(off[0, 3]) and np.isnan(got[:, 0, 3]).all() and np.isnan(got[:, 2, 11]).all()
    assert not np.isnan(got[:, ~nan_pixels]).any()                                   # and nowhere else


def test_surface(gpu):
    src = R.case_stack(24, 5, 37, seed=3)
    t = torch.from_numpy(src).to(gpu)
    want = R.destripe_sort(src, 9)
    a = PJ.destripe(t)                                                               # size 9, the sort method
    assert _bits_equal(a.cpu().numpy(), want)
    assert torch.equal(PJ.destripe(t, 9, "sort"), a)                                 # two runs
    m, off = PJ.destripe(t, 5, "mean", return_offsets=True)
    assert torch.equal(PJ.destripe(t, 5, "mean"), m) and torch.equal(PJ.destripe(t, 5, "mean", True)[1], off)
    assert off.shape == (5, 37) and torch.equal(PJ.stripe_offsets(t, 5), off)         # the offsets alone
    assert _bits_equal(PJ.stripe_offsets(t).cpu().numpy(), R.destripe_mean(src, 9)[1])
    # another dtype, another layout, a tensor that requires grad, numpy's integers
    assert torch.equal(PJ.destripe(t.double(), 9), a)
    tt = t.permute(0, 2, 1)
    assert torch.equal(PJ.destripe(tt, 5), PJ.destripe(tt.contiguous(), 5))
    assert torch.equal(PJ.destripe(t.clone().requires_grad_(True), np.int64(9)), a)
    # one projection [H,W] is one view: both methods then leave its median across the columns
    one = PJ.destripe(t[1], 3)
    assert one.shape == (5, 37) and _bits_equal(one.cpu().numpy(), R.destripe_sort(src[1], 3))
    assert _bits_equal(PJ.destripe(t[1], 3, "mean").cpu().numpy(), R.destripe_mean(src[1], 3)[0])
    # k = 1 is the identity
    assert torch.equal(PJ.destripe(t, 1), t) and torch.equal(PJ.destripe(t, 1, "mean"), t)
    assert not PJ.stripe_offsets(t, 1).any()
    # no views: nothing to do, and no offsets
    assert PJ.destripe(t[:0], 3).shape == (0, 5, 37) and PJ.destripe(t[:0], 3, "mean").shape == (0, 5, 37)
    with pytest.raises(ValueError):
        PJ.stripe_offsets(t[:0])
    # a NaN-filled, oversized workspace and a NaN-filled dst through the C ABI; without offsets; the offsets without dst
    L = _lib.lib()
    V, H, W = src.shape
    for method, name in ((0, "r2_proj_destripe_sort"), (1, "r2_proj_destripe_mean")):
        nbytes = int(L.r2_proj_destripe_workspace_bytes(V, H, W, method))
        assert nbytes == (V * H * W * 6 if method == 0 else H * W * 8)
        ws = torch.full((nbytes // 4 + 100,), float("nan"), device=gpu)
        dst = torch.full((V, H, W), float("nan"), device=gpu)
        extra = () if method == 0 else (None,)
        call(name, gpu, V, H, W, t, 9, dst, *extra, ws, ws.numel() * 4)
        assert torch.equal(dst, a if method == 0 else PJ.destripe(t, 9, "mean"))
    o = torch.full((H, W), float("nan"), device=gpu)
    call("r2_proj_destripe_mean", gpu, V, H, W, t, 5, None, o, ws, ws.numel() * 4)
    assert torch.equal(o, off)
    # V = 0 writes nothing
    dst.fill_(7.0)
    o.fill_(7.0)
    call("r2_proj_destripe_sort", gpu, 0, H, W, t, 9, dst, ws, ws.numel() * 4)
    call("r2_proj_destripe_mean", gpu, 0, H, W, t, 9, dst, o, ws, ws.numel() * 4)
    torch.cuda.synchronize()
    assert bool((dst == 7.0).all()) and bool((o == 7.0).all())


def test_no_host_sync(gpu):
    t = torch.from_numpy(R.case_stack(24, 5, 37, seed=3)).to(gpu)
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        a = PJ.destripe(t, 9)
        b, off = PJ.destripe(t, 9, "mean", return_offsets=True)
        c = PJ.stripe_offsets(t, 3)
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    assert a.shape == b.shape == t.shape and off.shape == c.shape == (5, 37)


def test_validation_before_any_launch(gpu):
    V, H, W = 6, 8, 12
    MAX_VIEWS = PJ.destripe_max_views()
    assert MAX_VIEWS == max(VIEWS_LONG) == int(_lib.lib().r2_proj_destripe_max_views())
    t = torch.rand(V, H, W, device=gpu)
    dst = torch.full((V, H, W), 7.0, device=gpu)
    off = torch.full((H, W), 7.0, device=gpu)
    L = _lib.lib()
    need = [int(L.r2_proj_destripe_workspace_bytes(V, H, W, m)) for m in (0, 1)]
    ws = torch.full((need[0] // 4,), 7.0, device=gpu)
    ok_sort = (V, H, W, t, 3, dst, ws, need[0])
    ok_mean = (V, H, W, t, 3, dst, off, ws, need[1])
    bad = []
    for i, v in ((0, -1), (0, MAX_VIEWS + 1), (1, 0), (2, -1), (3, None), (4, 0), (4, 4), (4, 33), (4, -1), (5, None), (6, None),
                 (7, need[0] - 1)):
        a = list(ok_sort)
        a[i] = v
        bad.append(("r2_proj_destripe_sort", tuple(a)))
    for i, v in ((0, -1), (1, 0), (2, 0), (3, None), (4, 2), (4, 35), (7, None), (8, need[1] - 1)):
        a = list(ok_mean)
        a[i] = v
        bad.append(("r2_proj_destripe_mean", tuple(a)))
    bad.append(("r2_proj_destripe_mean", (V, H, W, t, 3, None, None, ws, need[1])))
    bad.append(("r2_proj_destripe_sort", (2, 2 ** 16, 2 ** 15, t, 3, dst, ws, need[0])))
    bad.append(("r2_proj_destripe_mean", (2 ** 20, 2 ** 9, 2 ** 9, t, 3, dst, off, ws, need[1])))
    for name, args in bad:
        with pytest.raises(R2HipError):
            call(name, gpu, *args)
    # the Python surface
    for args, kw in (((t, 4), {}), ((t, 33), {}), ((t, 0), {}), ((t, 3, "sort", True), {}), ((t, 3), {"return_offsets": True}),
                     ((t, 3, "fourier"), {}), ((t[0, 0], 3), {}), ((t[None], 3), {}), ((t[:, :0], 3), {}),
                     ((torch.zeros(MAX_VIEWS + 1, 1, 1, device=gpu), 3), {})):
        with pytest.raises(ValueError):
            PJ.destripe(*args, **kw)
    with pytest.raises(ValueError):
        PJ.stripe_offsets(t, 6)
    for fn, args in ((PJ.destripe, (t.cpu(),)), (PJ.destripe, (t.cpu().numpy(),)), (PJ.stripe_offsets, (t.cpu(),))):
        with pytest.raises(R2HipError):
            fn(*args)
    assert PJ.destripe(torch.zeros(MAX_VIEWS + 1, 1, 1, device=gpu), 3, "mean").shape == (MAX_VIEWS + 1, 1, 1)
    torch.cuda.synchronize()
    assert bool((dst == 7.0).all()) and bool((off == 7.0).all()) and bool((ws == 7.0).all())


# ---- the converter, end to end -------------------------------------------------------------------------------------------------

CONFIG = """[Geometry]
DistanceSourceDetector=553.74
DistanceSourceOrigin=210.66
[CT]
NumberImages=24
AngleInterval=15.0
AngleFirst=0.0
AngleLast=345.0
[Detector]
PixelSize=0.8
PixelSizeUnit=mm
"""
DRIVER_ARGS = ["--proj_subsample", "2", "--n_train", "6", "--n_test", "4", "--nVoxel", "8", "8", "8", "--batch", "7"]


def _scan(folder):
    """24 measured projections of 40 x 48 in detector units, one per .npy file: a disc on a noisy background, and detector
    columns 20 and 21 (column 8 of the converted 20 x 20 projections) read 3 units too much in every view."""
    rng = np.random.RandomState(12)
    yy, xx = np.mgrid[:40, :48]
    disc = 24.0 * np.sqrt(np.maximum(0.0, 1.0 - ((yy - 22) / 13.0) ** 2 - ((xx - 24) / 15.0) ** 2))
    os.makedirs(folder)
    with open(os.path.join(folder, "config.txt"), "w") as f:
        f.write(CONFIG)
    images = []
    for i in range(24):
        img = disc * (1.0 + 0.05 * np.cos(i)) + rng.randn(40, 48) * 0.5 + 2.0
        img[:, 20:22] += 3.0
        np.save(os.path.join(folder, "scan_%03d.npy" % i), img)
        images.append(img)
    return images


def _stack_of(case, folder="proj_all"):
    return np.stack([np.load(os.path.join(case, folder, "scan_%03d.npy" % i)) for i in range(24)])


def test_converter_end_to_end(gpu, tmp_path):
    images = _scan(str(tmp_path / "scan"))
    plain = str(tmp_path / "plain")
    PR.main(["--data", str(tmp_path / "scan"), "--output", plain] + DRIVER_ARGS)
    # without the flag: byte for byte the files that the converter's pinned restatement gives
    for i, img in enumerate(images):
        buf = io.BytesIO()
        np.save(buf, PREF.real_projection(img, 400.0, 50, 2))
        with open(os.path.join(plain, "proj_all", "scan_%03d.npy" % i), "rb") as f:
            assert f.read() == buf.getvalue(), i
    before = _stack_of(plain)
    assert before.shape == (24, 20, 20)
    t = torch.from_numpy(before).to(gpu)
    for method in ("sort", "mean"):
        case = str(tmp_path / method)
        meta = PR.main(["--data", str(tmp_path / "scan"), "--output", case, "--destripe", "5", "--destripe_method", method] + DRIVER_ARGS)
        after = _stack_of(case)
        assert _bits_equal(after, PJ.destripe(t, 5, method).cpu().numpy()), method
        # the planted column is what changed most, and it came down by about the 3 / 400 * 50 that was planted
        change = (before - after)[:, :17].mean(axis=(0, 1))
        assert int(np.argmax(np.abs(change))) == 8 and 0.25 < change[8] < 0.5, (method, change)
        # the splits and the pseudo ground truth come from the destriped stack; the case loads
        with open(os.path.join(case, "meta_data.json")) as f:
            saved = json.load(f)
        assert saved == json.loads(json.dumps(meta))
        with open(os.path.join(plain, "meta_data.json")) as f:
            assert saved == json.load(f)
        for split in ("proj_train", "proj_test"):
            assert len(saved[split]) == (6 if split == "proj_train" else 4)
            for e in saved[split]:
                assert np.array_equal(np.load(os.path.join(case, e["file_path"])),
                                      np.load(os.path.join(case, "proj_all", os.path.basename(e["file_path"]))))
        angles = PR.scan_angles(PR.parse_config(os.path.join(str(tmp_path / "scan"), "config.txt"), 2, 50))
        want_vol = PR.F.fdk(after, angles, saved["scanner"]).clamp_min(0.0).cpu().numpy()
        assert np.array_equal(np.load(os.path.join(case, "vol_gt.npy")), want_vol)
        assert not np.array_equal(want_vol, np.load(os.path.join(plain, "vol_gt.npy")))
        c = recon._read_case(case)
        assert c["vol"].shape == (8, 8, 8) and c["train"][0].shape == (6, 20, 20) and c["test"][0].shape == (4, 20, 20)
    # bands of detector rows: rows are independent
    for method in ("sort", "mean"):
        want = PJ.destripe(t, 5, method).cpu().numpy()
        assert _bits_equal(PR.destripe_rows(before, 5, method, gpu, rows=3), want)
        assert _bits_equal(PR.destripe_rows(before, 5, method, gpu), want)
