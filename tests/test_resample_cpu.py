"""CPU: the restatement of the spline resampling entries (tests/resample_ref.py) against scipy's own results
(tests/golden/resample, and live scipy where it imports), output shapes at the half-way cases, the helpers' arithmetic, the
raw-data driver end to end, and the new entries in the header and the binding."""
import json
import os
import re

import numpy as np
import pytest

from r2_gaussian_amd import _lib
from r2_gaussian_amd import prepare as PR
from r2_gaussian_amd import resample as RS
from tests import resample_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "resample")
ZOOMS = [(shape, f) for shape, fs in R.ZOOM_CASES for f in fs]
_ZIDS = ["%s*%s" % ("x".join(map(str, s)), R.factor_id(f)) for s, f in ZOOMS]


def _gold(kind, key):
    return np.load(os.path.join(GOLD, "%s_%s.npz" % (kind, key if isinstance(key, str) else "x".join(map(str, key)))))


def _rel(got, want):
    return float(np.abs(got - want).max() / np.abs(want).max())


@pytest.mark.parametrize("shape,f", ZOOMS, ids=_ZIDS)
def test_float64_zoom_equals_scipys(shape, f):
    d = _gold("zoom", shape)
    assert np.array_equal(d["vol"], R.case_volume(shape))
    want = d["zoom_" + R.factor_id(f)]
    got = R.zoom(d["vol"], f)
    assert got.shape == want.shape == R.out_shape(shape, f) == RS.output_shape(shape, f)
    assert _rel(got, want) < 1e-12


@pytest.mark.parametrize("shape", R.SAMPLE_SHAPES, ids=str)
def test_float64_sampler_equals_scipys(shape):
    d = _gold("sample", shape)
    assert np.array_equal(d["points"], R.case_points(shape))
    got = R.map_coordinates(d["vol"], d["points"].astype(np.float64))
    assert _rel(got, d["values"]) < 1e-12
    # on the lattice nodes the spline interpolates the volume
    nodes = np.stack(np.meshgrid(*[np.arange(k) for k in shape], indexing="ij"), -1).reshape(-1, 3)
    assert np.abs(R.map_coordinates(d["vol"], nodes) - d["vol"].reshape(-1)).max() < 1e-12


@pytest.mark.parametrize("mode", [None, "crop", "expand"], ids=str)
def test_float64_reshape_vol_equals_the_references(mode):
    d = _gold("reshape", str(mode))
    got = R.reshape_vol(d["vol"].astype(np.float64), d["spacing"], int(d["target"]), mode)
    assert got.shape == d["out"].shape == (8, 8, 8)
    assert _rel(got, d["out"]) < 1e-12


def test_float64_restatement_against_live_scipy():
    ndimage = pytest.importorskip("scipy.ndimage")
    rng = np.random.RandomState(5)
    for shape, f in [((7, 5, 9), 2.2), ((13, 4, 6), (0.4, 1.5, 0.7)), ((2, 3, 1), (3.0, 0.4, 2.0)), ((20, 17, 33), 0.45)]:
        v = rng.rand(*shape)
        assert _rel(R.zoom(v, f), ndimage.zoom(v, f, mode="nearest")) < 1e-12, (shape, f)
    v = rng.rand(6, 5, 7)
    p = np.concatenate([rng.rand(500, 3) * 50 - 20, R.case_points((6, 5, 7)).astype(np.float64)])
    assert _rel(R.map_coordinates(v, p), ndimage.map_coordinates(v, p.T, order=3, mode="nearest")) < 1e-12
    assert _rel(R.prefilter(v), ndimage.spline_filter(np.pad(v, 12, mode="edge"), order=3, mode="nearest")) < 1e-12


def test_float32_restatement_stays_within_its_measured_bound():
    """Maximum absolute error of the float32 restatement against scipy's float64 fixtures over all listed cases, on U[0,1)
    data: measured 5.13e-7 (zoom 3.8e-7, sampler 5.13e-7, reshape_vol chains 2.9e-7).  The bound is four times that."""
    worst = {}
    for shape, f in ZOOMS:
        d = _gold("zoom", shape)
        got = R.zoom(d["vol"], f, np.float32)
        assert got.dtype == np.float32
        worst["zoom"] = max(worst.get("zoom", 0.0), float(np.abs(got - d["zoom_" + R.factor_id(f)]).max()))
    for shape in R.SAMPLE_SHAPES:
        d = _gold("sample", shape)
        got = R.map_coordinates(d["vol"], d["points"], np.float32)
        worst["sample"] = max(worst.get("sample", 0.0), float(np.abs(got - d["values"]).max()))
    for shape, spacing, target, mode in R.RESHAPE_CASES:
        d = _gold("reshape", str(mode))
        got = R.reshape_vol(d["vol"], spacing, target, mode, R.zoom32)
        worst["reshape"] = max(worst.get("reshape", 0.0), float(np.abs(got - d["out"]).max()))
    print("float32 restatement vs scipy float64:", worst)
    assert max(worst.values()) < R.F32_BOUND, worst


def test_output_shapes_round_half_to_even_as_scipy_does():
    assert RS.output_shape((5, 7, 3), 0.5) == (2, 4, 2) == R.out_shape((5, 7, 3), 0.5)      # 2.5 -> 2, 3.5 -> 4, 1.5 -> 2
    assert RS.output_shape((3, 3, 3), 1.5) == (4, 4, 4)                                     # 4.5 -> 4
    assert RS.output_shape((5, 7, 3), (0.5, 0.5, 1.5)) == (2, 4, 4)
    with pytest.raises(ValueError):
        RS.output_shape((5, 7, 3), (0.5, 0.5))


def test_constants_and_the_truncated_start():
    z = np.sqrt(3.0) - 2.0
    assert abs(R.GAIN - 6.0) < 1e-14 and np.float32(R.GAIN) == np.float32(6.0)
    assert abs(z) ** (R.HORIZON + 1) < 2.0 ** -32 and abs(z) ** 25 < 2.0 ** -47
    assert R.PAD == _lib.R2_SPLINE_PAD == 12 and R.HORIZON == _lib.R2_SPLINE_HORIZON == 16
    # a constant volume is reproduced: the coefficients of a constant are that constant
    c = R.prefilter(np.full((3, 2, 4), 0.7))
    assert np.abs(c - 0.7).max() < 1e-14


def test_helpers_follow_the_references_arithmetic():
    import torch
    v = np.arange(4 * 7 * 5, dtype=np.float32).reshape(4, 7, 5)
    e = R.expand_to_cube(v)
    assert e.shape == (7, 7, 7)
    # differences 3, 0, 2: one voxel before and two after along x, one and one along z
    assert np.array_equal(e[1:5, :, 1:6], v) and e[0].max() == 0 and e[5:].max() == 0 and e[:, :, 0].max() == 0 and e[:, :, 6].max() == 0
    c = R.crop_to_cube(v)
    assert np.array_equal(c, v[:, 1:5, 0:4])                                                # offsets 0, (7 - 4) // 2 = 1, (5 - 4) // 2 = 0
    # the product's helpers refuse host data: there is no CPU path
    for fn, args in ((RS.expand_to_cube, ()), (RS.crop_to_cube, ()), (RS.zoom, (2.0,)), (RS.spline_filter, ()),
                     (RS.resize, (8,)), (RS.resample, ((1, 1, 1),)), (RS.reshape_vol, ((1, 1, 1), 8))):
        with pytest.raises(_lib.R2HipError):
            fn(torch.zeros(3, 4, 5), *args)
        with pytest.raises(_lib.R2HipError):
            fn(np.zeros((3, 4, 5), np.float32), *args)
    with pytest.raises(_lib.R2HipError):
        RS.map_coordinates(torch.zeros(3, 4, 5), torch.zeros(2, 3))
    for fn, args in ((RS.zoom, (None, 2.0)), (RS.spline_filter, (None,)), (RS.map_coordinates, (None, None))):
        with pytest.raises(ValueError):
            fn(*args, order=1)
    # resample's shape arithmetic: round(shape * spacing), then the factor that reaches it
    new_shape = np.round(np.array([9, 6, 11]) * np.array([1.3, 0.8, 1.1]))
    assert list(new_shape) == [12, 5, 12]
    out, sp = R.resample(R.case_volume((9, 6, 11)).astype(np.float64), (1.3, 0.8, 1.1))
    assert out.shape == (12, 5, 12) and np.allclose(sp, np.array([1.3, 0.8, 1.1]) * np.array([9, 6, 11]) / new_shape)


def _write_case(tmp_path, ext):
    shape = [6, 5, 7]
    rng = np.random.RandomState(3)
    raw = rng.randint(0, 4000, size=shape[::-1]).astype(np.uint16)       # the file is [z][y][x], x fastest
    raw.tofile(str(tmp_path / "scan.raw"))
    info = [dict(raw_path=str(tmp_path / "scan.raw"), output_name="0_scan", file_type="raw", dtype="uint16", shape=shape,
                 spacing=[1.0, 1.2, 0.9], reshape="expand", transpose=[1, 0, 2], z_invert=True)]
    meta = str(tmp_path / ("meta" + ext))
    if ext == ".py":
        with open(meta, "w") as f:
            f.write("raw_info = %r\n" % (info,))
    elif ext == ".json":
        with open(meta, "w") as f:
            json.dump({"raw_info": info}, f)
    else:
        import yaml
        with open(meta, "w") as f:
            yaml.safe_dump(info, f)
    return raw, info, meta


@pytest.mark.parametrize("ext", [".py", ".json", ".yml"])
def test_driver_end_to_end_on_a_raw_file(tmp_path, monkeypatch, ext):
    """The driver's own steps -- reading, normalising, transposing, flipping, skipping, saving -- with the device resampler
    replaced by its float32 restatement (tests/test_resample_gpu.py runs the same case on the device)."""
    raw, info, meta = _write_case(tmp_path, ext)
    assert PR.load_metadata(meta) == info
    calls = []

    def reshape(data, spacing, target_size, mode, device):
        calls.append((data.shape, tuple(spacing), target_size, mode))
        return R.reshape_vol(np.asarray(data, np.float32), spacing, target_size, mode, R.zoom32).clip(0.0, 1.0)

    monkeypatch.setattr(PR, "_reshape", reshape)
    out = str(tmp_path / "volume_gt")
    PR.main(["--metadata", meta, "--output", out, "--target_size", "8"])
    got = np.load(os.path.join(out, "0_scan.npy"))
    assert got.dtype == np.float32 and got.shape == (8, 8, 8) and got.min() >= 0.0 and got.max() <= 1.0
    assert calls == [((6, 5, 7), (1.0, 1.2, 0.9), 8, "expand")]
    data = raw.astype(float).transpose(2, 1, 0)
    data = ((data - data.min()) / (data.max() - data.min())).clip(0.0, 1.0)
    want = R.reshape_vol(data.astype(np.float32), [1.0, 1.2, 0.9], 8, "expand", R.zoom32).clip(0.0, 1.0)
    assert np.array_equal(got, want.transpose(1, 0, 2)[:, :, ::-1])
    # an existing output is kept
    PR.main(["--metadata", meta, "--output", out, "--target_size", "8"])
    assert len(calls) == 1


def test_driver_file_types(tmp_path, monkeypatch):
    monkeypatch.setattr(PR, "_reshape", lambda data, spacing, target, mode, device: np.asarray(data, np.float32))
    v = np.random.RandomState(0).rand(3, 4, 5)
    np.save(str(tmp_path / "v.npy"), v)
    info = dict(raw_path=str(tmp_path / "v.npy"), output_name="a", file_type="npy", spacing=[1, 1, 1], reshape=None,
                transpose=[2, 0, 1], z_invert=False)
    PR.prepare([info], str(tmp_path / "o"), 4, verbose=False)
    want = ((v - v.min()) / (v.max() - v.min())).astype(np.float32).transpose(2, 0, 1)
    assert np.array_equal(np.load(str(tmp_path / "o" / "a.npy")), want)
    with pytest.raises(ValueError):
        PR.prepare([dict(info, output_name="b", file_type="mhd")], str(tmp_path / "o"), 4, verbose=False)
    for kind, module in (("tif", "tifffile"), ("dcm", "pydicom")):
        try:
            __import__(module)
        except ImportError:
            with pytest.raises(RuntimeError, match=module):
                PR.prepare([dict(info, output_name=kind, file_type=kind, thickness=None, xy_invert=False)], str(tmp_path / "o"), 4,
                           verbose=False)


def test_entries_are_declared_and_bound():
    with open(os.path.join(ROOT, "include", "r2hip.h")) as f:
        header = f.read()
    assert re.search(r"#define R2_ABI_VERSION 3\b", header) and _lib.R2_ABI_VERSION == 3
    syms = _lib.exported_symbols()
    for name, nargs in (("r2_spline_prefilter", 6), ("r2_spline_prefilter_pass", 7), ("r2_spline_zoom_workspace_bytes", 3),
                        ("r2_spline_zoom", 11), ("r2_spline_sample", 8)):
        m = re.search(r"R2_API (?:int|size_t) %s\(([^;]*)\);" % name, header)
        assert m, name
        assert len(re.sub(r"/\*.*?\*/", "", m.group(1)).split(",")) == nargs == len(_lib._SIGNATURES[name][1]), name
        assert name in syms
    L = _lib.lib()
    assert L.r2_abi_version() == 3
    assert L.r2_spline_zoom_workspace_bytes(3, 4, 5) == 12 * 20 and L.r2_spline_zoom_workspace_bytes(0, 4, 5) == 0
    for name in ("spline_filter", "zoom", "map_coordinates", "resample", "resize", "crop_to_cube", "expand_to_cube", "reshape_vol"):
        assert callable(getattr(RS, name)), name
