"""The stripe-removal restatement (tests/destripe_ref.py, what tests/test_destripe_gpu.py holds the kernels to) against facts that
share nothing with it: a brute-force sort in plain Python, exact identities of the two methods, and one quality condition on an
analytic sinogram.  Also here, because they need no device: the synthetic defect of ``datagen --stripes``, the refusals of the
Python surface, and the library's refusals before any launch."""
import json
import os

import numpy as np
import pytest
import torch

from r2_gaussian_amd import _lib
from r2_gaussian_amd import datagen as DG
from r2_gaussian_amd import prepare_real as PR
from r2_gaussian_amd import projections as PJ
from r2_gaussian_amd._lib import R2HipError
from tests import destripe_ref as R

F32 = np.float32


def _bits_equal(got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    return got.dtype == want.dtype == np.float32 and got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32))


def _columnwise(V, H, seed):
    """A stack that is constant along the detector columns: multiples of 2^-10 in [0, 1), so that adding 0.25 is exact."""
    rng = np.random.RandomState(seed)
    return (rng.randint(0, 1024, size=(V, H, 1)) / 1024.0).astype(F32)


# ---- the restatement against plain Python --------------------------------------------------------------------------------------

def _brute_sort(x, k):
    V, H, W = x.shape
    out = np.empty_like(x)
    for h in range(H):
        cols = []
        for w in range(W):
            col = [float("inf") if np.isnan(x[v, h, w]) else float(x[v, h, w]) for v in range(V)]
            cols.append(sorted(range(V), key=lambda v: (col[v], v)))       # views by (value, view)
        for w in range(W):
            for r in range(V):
                window = []
                for j in range(-(k // 2), k // 2 + 1):
                    wj = min(max(w + j, 0), W - 1)
                    v = cols[wj][r]
                    window.append(float("inf") if np.isnan(x[v, h, wj]) else float(x[v, h, wj]))
                out[cols[w][r], h, w] = sorted(window)[k // 2]
    return out


def _brute_mean(x, k):
    V, H, W = x.shape
    d = np.empty((H, W), F32)
    for h in range(H):
        m = []
        for w in range(W):
            acc = 0.0                                                      # a Python float is a double
            for v in range(V):
                acc = acc + float(x[v, h, w])
            m.append(F32(acc / V))
        for w in range(W):
            window = sorted(float("inf") if np.isnan(m[min(max(w + j, 0), W - 1)]) else float(m[min(max(w + j, 0), W - 1)])
                            for j in range(-(k // 2), k // 2 + 1))
            d[h, w] = m[w] - F32(window[k // 2])
    return x - d[None], d


@pytest.mark.parametrize("k", [1, 3, 5, 9])
def test_restatement_equals_a_brute_force_in_plain_python(k):
    rng = np.random.RandomState(k)
    x = np.round(rng.randn(9, 2, 7) * 2.0).astype(F32) / F32(2)            # nine levels or so: ties everywhere
    x[3, 0, 2] = np.nan
    x[:, 1, 5] = np.nan
    x[4, 1, 1] = np.inf
    assert np.array_equal(R.destripe_sort(x, k), _brute_sort(x, k))        # numeric: -0 and +0 tie
    y = R.case_stack(9, 2, 7)
    y[2, 1, 3] = np.nan
    with np.errstate(invalid="ignore"):
        want, want_d = _brute_mean(y, k)
    got, got_d = R.destripe_mean(y, k)
    assert np.array_equal(got, want, equal_nan=True) and np.array_equal(got_d, want_d, equal_nan=True)
    assert np.isnan(got[:, 1, 3]).all() and np.isnan(got_d[1, 3]) and np.isnan(got).sum() == 9       # a NaN takes its pixel only


# ---- exact identities ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [3, 9, 31])
def test_a_stack_constant_along_the_columns_comes_back_and_an_added_constant_goes(k):
    V, H, W = 50, 3, 40
    flat = np.broadcast_to(_columnwise(V, H, 1), (V, H, W)).copy()
    assert _bits_equal(R.destripe_sort(flat, k), flat)
    dst, d = R.destripe_mean(flat, k)
    assert _bits_equal(dst, flat) and not d.any()
    striped = flat.copy()
    striped[:, :, 17] += F32(0.25)                                         # exact: no tie appears or disappears
    striped[:, 1, 1] += F32(0.25)                                          # next to the border, one row only
    assert _bits_equal(R.destripe_sort(striped, k), flat)
    # The mean method leaves at most one ulp of the offset, 2^-25 for 0.25: the two means that meet in d are rounded to float32
    # once each, so in general more can stay; on this stack nothing does.
    ulp = 2.0 ** -25
    dst, d = R.destripe_mean(striped, k)
    assert np.abs(dst.astype(np.float64) - flat).max() <= ulp
    assert np.abs(d[:, 17].astype(np.float64) - 0.25).max() <= ulp and abs(float(d[1, 1]) - 0.25) <= ulp
    off = np.ones((H, W), bool)
    off[:, 17] = off[1, 1] = False
    assert not d[off].any()


def test_permuting_the_views_permutes_the_sorted_result():
    x = R.case_stack(40, 2, 30)
    assert all(len(np.unique(x[:, h, w])) == 40 for h in range(2) for w in range(30))      # tie-free
    perm = np.random.RandomState(2).permutation(40)
    for k in (3, 11):
        assert _bits_equal(R.destripe_sort(x[perm], k), R.destripe_sort(x, k)[perm])


def test_a_window_of_one_is_the_identity():
    x = R.case_stack(20, 3, 11)
    assert _bits_equal(R.destripe_sort(x, 1), x)
    dst, d = R.destripe_mean(x, 1)
    assert _bits_equal(dst, x) and not d.any()
    one = R.destripe_sort(x[0], 3)                                         # [H,W] is one view
    assert one.shape == (3, 11) and _bits_equal(one, R.destripe_sort(x[:1], 3)[0])


# ---- quality -------------------------------------------------------------------------------------------------------------------

def test_stripes_of_an_analytic_sinogram_lose_more_than_half_of_their_error():
    """Four ellipses, 360 x 2 x 256, noise 0.005, 16 columns with offsets from N(0, 0.05), k = 11: the RMS error against the clean
    sinogram on those columns falls from 0.0503 to 0.0141 (sort, 0.28 of it) and 0.0116 (mean, 0.23); the condition is below
    one half."""
    clean = R.ellipse_sinogram(360, 2, 256)
    rng = np.random.RandomState(7)
    noisy = clean + rng.randn(*clean.shape) * 0.005
    cols = np.sort(rng.choice(256, size=16, replace=False))
    offsets = rng.normal(0.0, 0.05, size=(2, 16))
    striped = noisy.copy()
    striped[:, :, cols] += offsets[None]
    striped = striped.astype(F32)
    rms = lambda a: float(np.sqrt(np.mean((a[:, :, cols].astype(np.float64) - clean[:, :, cols]) ** 2)))   # noqa: E731
    before = rms(striped)
    for name, got in (("sort", R.destripe_sort(striped, 11)), ("mean", R.destripe_mean(striped, 11)[0])):
        ratio = rms(got) / before
        print("destripe quality, %s: RMS error on the striped columns %.5f -> %.5f, ratio %.3f" % (name, before, rms(got), ratio))
        assert ratio < 0.5, (name, ratio)


# ---- datagen --stripes ---------------------------------------------------------------------------------------------------------

def test_stripe_field_is_a_draw_of_its_own():
    cols, field = DG.stripe_field((6, 40), 5, 0.05, seed=3)
    cols2, field2 = DG.stripe_field((6, 40), 5, 0.05, seed=3)
    assert cols == cols2 == sorted(set(cols)) and len(cols) == 5 and all(isinstance(c, int) and 0 <= c < 40 for c in cols)
    assert field.dtype == np.float32 and field.shape == (6, 40) and np.array_equal(field, field2)
    other = np.ones(40, bool)
    other[cols] = False
    assert not field[:, other].any() and (field[:, cols] != 0).all()
    assert len(np.unique(field[:, cols])) == 30                            # one offset per (row, column)
    assert DG.stripe_field((6, 40), 5, 0.05, seed=4)[0] != cols
    assert DG.stripe_field((6, 40), 0, 0.05, seed=3)[0] == [] and not DG.stripe_field((6, 40), 40, 0.0, seed=3)[1].any()
    for n, amp in ((41, 0.1), (-1, 0.1), (2.5, 0.1), (3, -1.0), (3, float("nan"))):
        with pytest.raises(ValueError):
            DG.stripe_field((6, 40), n, amp, seed=0)


def test_generate_with_stripes_moves_no_other_draw(tmp_path, monkeypatch):
    """``generate`` on a stand-in projector that runs on the host: with ``stripes`` every file of the case is the file of the
    case without them, plus the field on the projections and the recorded columns."""
    cfg = {"mode": "cone", "nDetector": [6, 40], "noise": True, "possion_noise": 1e4, "gaussian_noise": [0, 10], "totalAngle": 360.0,
           "startAngle": 0.0}

    def project(vol, angles, cfg, device=None, projection_type=None):
        a = np.asarray(angles, dtype=np.float64)
        img = np.linspace(0.5, 1.5, 240).reshape(6, 40)
        return torch.from_numpy((img[None] * (2.0 + np.cos(a))[:, None, None]).astype(np.float32))

    monkeypatch.setattr(DG.P, "project", project)
    vol = np.zeros((4, 4, 4), np.float32)
    defects = dict(dead_pixels=0.05, dead_lines=1, gap=None)
    plain = DG.generate(vol, cfg, str(tmp_path / "plain"), "v", 5, 4, seed=9, defects=defects)
    again = DG.generate(vol, cfg, str(tmp_path / "again"), "v", 5, 4, seed=9, defects=defects, stripes=None)
    striped = DG.generate(vol, cfg, str(tmp_path / "striped"), "v", 5, 4, seed=9, defects=defects, stripes=(3, 0.05))
    cols, field = DG.stripe_field((6, 40), 3, 0.05, seed=9)

    def files(case):
        return sorted(os.path.relpath(os.path.join(d, f), case) for d, _, fs in os.walk(case) for f in fs)

    def read(case, name):
        with open(os.path.join(case, name), "rb") as f:
            return f.read()

    assert files(plain) == files(again) == files(striped)
    for name in files(plain):
        assert read(plain, name) == read(again, name), name                # without the flag: byte for byte
    with open(os.path.join(striped, "meta_data.json")) as f:
        meta = json.load(f)
    with open(os.path.join(plain, "meta_data.json")) as f:
        meta_plain = json.load(f)
    assert "stripe_columns" not in meta_plain and meta.pop("stripe_columns") == cols and meta == meta_plain
    mask = np.load(os.path.join(plain, "weights_train.npy"))
    assert np.array_equal(np.load(os.path.join(striped, "weights_train.npy")), mask) and (mask == 0).any()
    for e in meta["proj_train"]:
        a, b = np.load(os.path.join(plain, e["file_path"])), np.load(os.path.join(striped, e["file_path"]))
        assert b.dtype == np.float32 and np.array_equal(b, np.where(mask > 0, a + field, F32(0)))   # the same noise, test angles, mask
    for e in meta["proj_test"]:
        a, b = np.load(os.path.join(plain, e["file_path"])), np.load(os.path.join(striped, e["file_path"]))
        assert np.array_equal(b, a + field)
    assert np.array_equal(np.load(os.path.join(striped, "vol_gt.npy")), np.load(os.path.join(plain, "vol_gt.npy")))


# ---- refusals ------------------------------------------------------------------------------------------------------------------

def test_parser_defaults_leave_the_stripes_alone():
    a = PR.parser().parse_args(["--data", "in", "--output", "out"])
    assert a.destripe is None and a.destripe_method == "sort"
    a = PR.parser().parse_args(["--data", "in", "--output", "out", "--destripe", "9", "--destripe_method", "mean"])
    assert a.destripe == 9 and a.destripe_method == "mean"
    for bad in ("4", "33", "-1"):
        with pytest.raises(SystemExit):
            PR.main(["--data", "in", "--output", "out", "--destripe", bad])


def test_host_tensors_and_bad_arguments_are_refused():
    x = torch.rand(4, 8, 12)
    for fn, args in ((PJ.destripe, (x,)), (PJ.destripe, (x.numpy(), 3)), (PJ.destripe, (x, 3, "mean", True)), (PJ.stripe_offsets, (x,))):
        with pytest.raises(R2HipError):
            fn(*args)
    # arguments that do not depend on the projections are checked first: no tensor is touched, nothing is launched
    for fn, args, kw in ((PJ.destripe, (x, 4), {}), (PJ.destripe, (x, 33), {}), (PJ.destripe, (x, 0), {}), (PJ.destripe, (x, True), {}),
                         (PJ.destripe, (x, 3.0), {}), (PJ.destripe, (x, 3, "median"), {}),
                         (PJ.destripe, (x, 3), {"return_offsets": True}), (PJ.destripe, (x, 3, "sort", True), {}),
                         (PJ.stripe_offsets, (x, 2), {})):
        with pytest.raises(ValueError):
            fn(*args, **kw)


def test_the_library_refuses_before_any_launch():
    """R2_ERR_INVALID comes back before the first launch, so these calls need no GPU: the pointers are never followed."""
    L = _lib.lib()
    p = 4096                                                               # a stand-in for device pointers
    assert PJ.destripe_max_views() == L.r2_proj_destripe_max_views() == 4096              # R2_DESTRIPE_MAX_VIEWS of the header
    assert L.r2_proj_destripe_workspace_bytes(5, 8, 12, 0) == 5 * 8 * 12 * 6 and L.r2_proj_destripe_workspace_bytes(5, 8, 12, 1) == 8 * 12 * 8
    for V, H, W, method in ((-1, 8, 12, 0), (5, 0, 12, 1), (5, 8, 0, 0), (5, 8, 12, 2), (5, 8, 12, -1), (4097, 1, 1, 0),
                            (2, 2 ** 16, 2 ** 15, 1), (2 ** 20, 2 ** 9, 2 ** 9, 1)):
        assert L.r2_proj_destripe_workspace_bytes(V, H, W, method) == 0, (V, H, W, method)
    assert L.r2_proj_destripe_workspace_bytes(4097, 1, 1, 1) == 8
    ok = dict(V=5, H=8, W=12, src=p, k=3, dst=p, offsets=p, ws=p, ws_bytes=1 << 20)
    bad = [dict(V=-1), dict(H=0), dict(W=-2), dict(k=0), dict(k=2), dict(k=33), dict(k=-3), dict(src=None), dict(ws=None),
           dict(H=2 ** 16, W=2 ** 15), dict(V=2 ** 20, H=2 ** 9, W=2 ** 9)]
    for change in bad + [dict(dst=None), dict(V=4097, H=1, W=1), dict(ws_bytes=5 * 8 * 12 * 6 - 1)]:
        a = dict(ok, **change)
        rc = L.r2_proj_destripe_sort(*[a[n] for n in ("V", "H", "W", "src", "k", "dst", "ws", "ws_bytes")], None)
        assert rc == _lib.R2_ERR_INVALID and L.r2_last_error(), change
    for change in bad + [dict(dst=None, offsets=None), dict(ws_bytes=8 * 12 * 8 - 1)]:
        a = dict(ok, **change)
        rc = L.r2_proj_destripe_mean(*[a[n] for n in ("V", "H", "W", "src", "k", "dst", "offsets", "ws", "ws_bytes")], None)
        assert rc == _lib.R2_ERR_INVALID and L.r2_last_error(), change
    # V = 0 is a no-op, whatever the pointers
    assert L.r2_proj_destripe_sort(0, 8, 12, None, 3, None, None, 0, None) == 0
    assert L.r2_proj_destripe_mean(0, 8, 12, None, 3, None, None, None, 0, None) == 0
