"""CPU: the host side of the weighted image loss -- the float64 restatement (tests/weighted_loss_ref.py) against central
differences, the C ABI's four new entries in the header and the ctypes table, the wrappers' shape checks (before anything
touches the library or a device), the defect masks and the fill of weights.py, the case layout's ``weights_train`` and the
trainer's flag."""
import filecmp
import os

import numpy as np
import pytest
import torch

from tests import loss_ref as R
from tests import weighted_loss_ref as WR
from tests.test_abi_cpu import declared_symbols

SHAPES = [(5, 7), (17, 15), (33, 31)]


def _content(hw, seed=0):
    """Random non-negative image and measurement, random weights with 30 % zeros, NaN measurements under the zeros."""
    rng = np.random.default_rng(hw[0] * 131 + hw[1] + seed)
    y = rng.random(hw)
    x = np.clip(y + 0.1 * rng.standard_normal(hw), 0, None)
    w = (2.0 * rng.random(hw) + 1e-3) * (rng.random(hw) > 0.3)
    y_nan = y.copy()
    y_nan[w == 0] = np.nan
    return x, y, y_nan, w


@pytest.mark.parametrize("hw", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_reference_gradient_against_central_differences(hw):
    x, _y, y_nan, w = _content(hw)
    ref = WR.weighted_l1_ssim64(x, y_nan, w)
    assert np.isfinite(ref["grad"]).all() and np.isfinite(ref["loss"])
    assert WR.weighted_bounds(ref)["cond_ok"]
    yp, sw = ref["yp"], ref["sum_w"]

    def loss(xx):       # y' is a constant copy of x: not differentiated
        r = R.l1_ssim64(xx, yp, 1.0, 0.25)
        return (ref["w"] * np.abs(xx - yp)).sum() / sw + 0.25 * (1.0 - (ref["w"] * r["S"]).sum() / sw)

    assert abs(loss(x) - ref["loss"]) <= 1e-14
    rng = np.random.default_rng(1)
    h, worst = 1e-6, 0.0
    pixels = {(int(rng.integers(hw[0])), int(rng.integers(hw[1]))) for _ in range(30)}
    pixels |= {tuple(int(v) for v in p) for p in np.argwhere(ref["w"] == 0)[:5]}     # unmeasured pixels too
    for i, j in pixels:
        xp, xm = x.copy(), x.copy()
        xp[i, j] += h
        xm[i, j] -= h
        worst = max(worst, abs((loss(xp) - loss(xm)) / (2 * h) - ref["grad"][i, j]))
    assert worst <= 1e-8, worst


@pytest.mark.parametrize("hw", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_unit_weights_reproduce_the_unweighted_reference(hw):
    x, y, _y_nan, _w = _content(hw)
    base = R.l1_ssim64(x, y, 1.0, 0.25)
    for weights in (None, np.ones(hw)):
        ref = WR.weighted_l1_ssim64(x, y, weights)
        assert ref["loss"] == base["loss"] and ref["l1"] == base["l1"] and ref["ssim"] == base["ssim"]
        assert np.array_equal(ref["grad"], base["grad"]) and ref["sum_w"] == x.size


def test_reference_weight_rules():
    x, y, y_nan, w = _content((17, 15))
    ref = WR.weighted_l1_ssim64(x, y_nan, w)
    bad = w.copy()
    bad[w == 0] = np.where(np.arange((w == 0).sum()) % 2 == 0, -3.0, np.nan)       # negative and NaN weights are zeros
    other = WR.weighted_l1_ssim64(x, y, bad)
    assert other["loss"] == ref["loss"] and np.array_equal(other["grad"], ref["grad"])
    none = WR.weighted_l1_ssim64(x, y_nan, np.zeros_like(w))
    assert (none["loss"], none["l1"], none["ssim"], none["sum_w"]) == (0.0, 0.0, 1.0, 0.0) and not none["grad"].any()
    b = WR.weighted_bounds(none)
    assert b["loss"] == 0.0 and not b["grad"].any()


def test_weighted_entries_are_declared_and_bound():
    from r2_gaussian_amd import _lib
    counts = {"r2_loss_l1_ssim_weighted_scratch_floats": 2, "r2_loss_l1_ssim_weighted": 11,
              "r2_loss_l1_ssim_weighted_batch_scratch_floats": 3, "r2_loss_l1_ssim_weighted_batch": 12}
    for name, n in counts.items():
        assert name in declared_symbols(), name
        assert name in _lib.exported_symbols(), name
        assert len(_lib._SIGNATURES[name][1]) == n, name
    assert _lib.R2_ABI_VERSION == 3          # the entries are additive


def test_wrappers_reject_bad_weight_shapes_before_the_library(monkeypatch):
    from r2_gaussian_amd import _lib, losses

    def no_library():
        raise AssertionError("the library was touched before the shapes were checked")
    monkeypatch.setattr(_lib, "lib", no_library)
    img, gt = torch.zeros(1, 8, 10), torch.zeros(8, 10)
    for w in (torch.zeros(8, 11), torch.zeros(10, 8), torch.zeros(2, 8, 10), torch.zeros(80), torch.zeros(1, 1, 8, 10),
              np.zeros((8, 10)), torch.zeros(8, 10, dtype=torch.complex64)):
        with pytest.raises(ValueError):
            losses.image_loss(img, gt, 0.25, weights=w)
    imgs = torch.zeros(3, 8, 10)
    gts = [torch.zeros(8, 10)] * 3
    ok = torch.ones(8, 10)
    bad = [torch.zeros(2, 8, 10), torch.zeros(3, 10, 8), torch.zeros(8, 10), [ok, ok], [ok, None, torch.zeros(8, 11)],
           [ok, None, torch.zeros(3, 8, 10)], [ok, ok, 1.0], []]
    for w in bad:
        with pytest.raises(ValueError):
            losses.image_loss_batch(imgs, gts, 0.25, weights=w)
    with pytest.raises(ValueError):
        losses.image_loss_batch(imgs, gts[:2], 0.25, weights=[ok, ok, ok])       # the existing checks still come first
    # good shapes on CPU tensors get past the shape checks and are refused as such: there is no CPU fallback
    monkeypatch.undo()
    with pytest.raises(_lib.R2HipError):
        losses.image_loss(img, gt, 0.25, weights=torch.ones(1, 8, 10, dtype=torch.bool))
    with pytest.raises(_lib.R2HipError):
        losses.image_loss_batch(imgs, gts, 0.25, weights=[ok, None, ok.double()])


# ------------------------------------------------------------------------------------------------------ weights.py
def test_defect_mask_is_deterministic_and_has_the_requested_counts():
    from r2_gaussian_amd.weights import defect_mask
    H, W = 24, 40
    m = defect_mask((H, W), np.random.RandomState(3), dead_pixels=0.05)
    assert m.shape == (H, W) and m.dtype == np.float32 and set(np.unique(m)) == {0.0, 1.0}
    assert int((m == 0).sum()) == round(0.05 * H * W)
    m = defect_mask((H, W), np.random.RandomState(3), dead_lines=5)
    rows, cols = (m == 0).all(axis=1), (m == 0).all(axis=0)
    assert rows.sum() + cols.sum() == 5
    assert int((m == 0).sum()) == rows.sum() * W + cols.sum() * H - rows.sum() * cols.sum()
    m = defect_mask((H, W), np.random.RandomState(3), gap=(10, 14))
    assert not m[:, 10:14].any() and m[:, :10].all() and m[:, 14:].all()
    kw = dict(dead_pixels=0.02, dead_lines=2, gap=(30, 33))
    a, b = defect_mask((H, W), np.random.RandomState(7), **kw), defect_mask((H, W), np.random.RandomState(7), **kw)
    assert np.array_equal(a, b) and not np.array_equal(a, defect_mask((H, W), np.random.RandomState(8), **kw))
    assert defect_mask((H, W), np.random.RandomState(0)).all()               # no defect asked for: all measured ...
    rng = np.random.RandomState(5)
    defect_mask((H, W), rng)
    assert rng.rand() == np.random.RandomState(5).rand()                      # ... and nothing drawn
    for bad in (dict(dead_pixels=1.5), dict(dead_lines=-1), dict(gap=(5, 5)), dict(gap=(0, W + 1))):
        with pytest.raises(ValueError):
            defect_mask((H, W), np.random.RandomState(0), **bad)


def test_fill_unmeasured_against_a_brute_force_loop():
    from r2_gaussian_amd.weights import fill_unmeasured
    rng = np.random.default_rng(2)
    H, W, radius = 9, 11, 2
    p = rng.random((3, H, W)).astype(np.float32)
    w = (rng.random((H, W)) > 0.4).astype(np.float32)
    w[:6, :6] = 0                                         # a hole wider than the window: its middle has no measured pixel
    w[7, 7] = np.nan                                      # not > 0: unmeasured
    dirty = p.copy()
    dirty[:, ~(w > 0)] = np.nan
    got = fill_unmeasured(dirty, w, radius)
    want = np.empty_like(p)
    for v in range(3):
        for i in range(H):
            for j in range(W):
                if w[i, j] > 0:
                    want[v, i, j] = p[v, i, j]
                    continue
                vals = [float(p[v, a, b]) for a in range(max(0, i - radius), min(H, i + radius + 1))
                        for b in range(max(0, j - radius), min(W, j + radius + 1)) if w[a, b] > 0]
                want[v, i, j] = sum(vals) / len(vals) if vals else 0.0
    assert got.dtype == np.float32 and np.isfinite(got).all()
    assert np.array_equal(got[:, w > 0].view(np.int32), p[:, w > 0].view(np.int32))          # measured: bit for bit
    assert np.allclose(got, want, rtol=1e-6, atol=0) and got[0, 2, 2] == 0.0
    assert np.array_equal(fill_unmeasured(dirty[0], w, radius), got[0])                      # one [H, W] projection
    per_view = np.stack([w, np.ones_like(w), w])
    got3 = fill_unmeasured(np.stack([dirty[0], p[1], dirty[2]]), per_view, radius)
    assert np.array_equal(got3[1], p[1]) and np.array_equal(got3[0], got[0])


# --------------------------------------------------------------------------------------------------- the case layout
def _tiny_case():
    rng = np.random.default_rng(0)
    cfg = {"mode": "cone", "DSD": 7.0, "DSO": 5.0, "nDetector": [6, 8], "sDetector": [3.0, 4.0], "nVoxel": [4, 4, 4],
           "sVoxel": [2.0, 2.0, 2.0], "offOrigin": [0, 0, 0], "offDetector": [0, 0], "possion_noise": 1e5,
           "gaussian_noise": [0, 10]}
    vol = rng.random((4, 4, 4)).astype(np.float32)
    train, test = rng.random((5, 6, 8)).astype(np.float32), rng.random((2, 6, 8)).astype(np.float32)
    return cfg, vol, train, np.linspace(0, 3, 5), test, np.array([0.5, 1.5])


def test_case_round_trips_weights_train(tmp_path):
    from r2_gaussian_amd import datagen, weights as WT
    from r2_gaussian_amd.recon import _read_case
    cfg, vol, train, ta, test, sa = _tiny_case()
    mask = WT.defect_mask(cfg["nDetector"], np.random.RandomState(1), dead_pixels=0.1, gap=(3, 5))
    meta = datagen.write_case(str(tmp_path / "c"), cfg, vol, np.where(mask > 0, train, 0), ta, test, sa, weights_train=mask)
    assert meta["weights_train"] == "weights_train.npy"
    case = _read_case(str(tmp_path / "c"))
    assert case["weights_train"].dtype == np.float32 and np.array_equal(case["weights_train"], mask)
    assert not case["train"][0][:, mask == 0].any()
    per_view = np.stack([mask] * 5)
    datagen.write_case(str(tmp_path / "v"), cfg, vol, train, ta, test, sa, weights_train=per_view)
    assert _read_case(str(tmp_path / "v"))["weights_train"].shape == (5, 6, 8)
    with pytest.raises(ValueError):
        datagen.write_case(str(tmp_path / "bad"), cfg, vol, train, ta, test, sa, weights_train=np.ones((6, 9)))
    # the trainer's modes
    assert np.array_equal(WT.resolve_weights(case, "auto"), mask) and np.array_equal(WT.resolve_weights(case, "file"), mask)
    assert WT.resolve_weights(case, "none") is None
    from r2_gaussian_amd.uncertainty import noise_weights
    nw = WT.resolve_weights(case, "noise")
    clean = np.where(mask > 0, case["train"][0], 0)
    assert nw.shape == (5, 6, 8) and not nw[:, mask == 0].any() and (nw[:, mask > 0] > 0).all()
    assert np.array_equal(nw[:, mask > 0], noise_weights(clean, 1e5, [0, 10])[:, mask > 0])
    nan_case = dict(case, train=(np.where(mask > 0, case["train"][0], np.nan).astype(np.float32), case["train"][1]))
    assert np.array_equal(WT.resolve_weights(nan_case, "noise"), nw)          # what an unmeasured pixel holds does not enter
    with pytest.raises(ValueError):
        WT.resolve_weights(case, "other")


def test_case_without_defects_is_byte_identical(tmp_path):
    from r2_gaussian_amd import datagen, weights as WT
    from r2_gaussian_amd.recon import _read_case
    cfg, vol, train, ta, test, sa = _tiny_case()
    datagen.write_case(str(tmp_path / "a"), cfg, vol, train, ta, test, sa)
    datagen.write_case(str(tmp_path / "b"), cfg, vol, train, ta, test, sa, weights_train=None)
    names = sorted(os.path.relpath(os.path.join(d, f), tmp_path / "a") for d, _, fs in os.walk(tmp_path / "a") for f in fs)
    assert names == sorted(os.path.relpath(os.path.join(d, f), tmp_path / "b") for d, _, fs in os.walk(tmp_path / "b") for f in fs)
    assert "weights_train.npy" not in names and len(names) == 2 + 5 + 2
    match, mismatch, errors = filecmp.cmpfiles(tmp_path / "a", tmp_path / "b", names, shallow=False)
    assert not mismatch and not errors and len(match) == len(names)
    case = _read_case(str(tmp_path / "a"))
    assert case["weights_train"] is None
    assert WT.resolve_weights(case, "auto") is None
    with pytest.raises(ValueError):
        WT.resolve_weights(case, "file")
    assert WT.resolve_weights(case, "noise").shape == (5, 6, 8)


def test_parsers_know_the_new_flags():
    from r2_gaussian_amd import train as TR
    ap = TR.build_parser()
    assert ap.parse_args(["-s", "x"]).loss_weights == "auto"
    for mode in ("auto", "none", "file", "noise"):
        assert ap.parse_args(["-s", "x", "--loss_weights", mode]).loss_weights == mode
    with pytest.raises(SystemExit):
        ap.parse_args(["-s", "x", "--loss_weights", "mask"])
