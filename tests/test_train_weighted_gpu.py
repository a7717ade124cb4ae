"""GPU: the native trainer (python -m r2_gaussian_amd.train) with per-pixel weights, end to end on cases written by datagen
with a detector gap and dead pixels: what the unmeasured pixels hold (0 or NaN) changes no bit of the trained model, unit
weights train to the bits of no weights, ``--loss_weights file`` needs recorded weights, and several views per step take them."""
import json
import os
import pickle
import shutil
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ITERS = 120
COMMON = ["--iterations", str(ITERS), "--densify_from_iter", "40", "--densify_until_iter", "100", "--densification_interval", "20",
          "--position_lr_max_steps", str(ITERS), "--density_lr_max_steps", str(ITERS), "--scaling_lr_max_steps", str(ITERS),
          "--rotation_lr_max_steps", str(ITERS), "--test_iterations", str(ITERS), "--quiet"]


def _blob(n, c0, sigma, rho):
    ax = -1 + (np.arange(n) + 0.5) * 2.0 / n
    X, Y, Z = np.meshgrid(ax, ax, ax, indexing="ij")
    return (rho * np.exp(-((X - c0[0]) ** 2 + (Y - c0[1]) ** 2 + (Z - c0[2]) ** 2) / (2 * sigma ** 2))).astype(np.float32)


def _copy_case(src, dst, weights=None, fill=None):
    """A copy of the case `src`; weights: recorded as its weights_train; fill: written into the training projections where the
    case's weights are 0."""
    shutil.copytree(src, dst)
    meta_path = os.path.join(dst, "meta_data.json")
    with open(meta_path) as f:
        meta = json.load(f)
    if weights is not None:
        np.save(os.path.join(dst, "weights_train.npy"), weights.astype(np.float32))
        meta["weights_train"] = "weights_train.npy"
        with open(meta_path, "w") as f:
            json.dump(meta, f, indent=4)
    if fill is not None:
        w = np.load(os.path.join(dst, meta["weights_train"]))
        for e in meta["proj_train"]:
            p = np.load(os.path.join(dst, e["file_path"]))
            p[w == 0] = fill
            np.save(os.path.join(dst, e["file_path"]), p)
    return dst


@pytest.fixture(scope="module")
def cases(tmp_path_factory, gpu):
    from r2_gaussian_amd import datagen as D
    from r2_gaussian_amd import scene as S
    n = 32
    vol = _blob(n, (0.1, -0.2, 0.05), 0.3, 0.6) + _blob(n, (-0.3, 0.25, -0.1), 0.15, 0.5)
    cfg = dict(S.CONE_BEAM, nVoxel=[n, n, n], nDetector=[64, 64], noise=False, totalAngle=360.0, startAngle=0.0)
    root = tmp_path_factory.mktemp("weighted")
    masked = D.generate(vol, cfg, str(root / "masked"), "phantom", n_train=20, n_test=4, seed=0,
                        defects=dict(dead_pixels=0.01, dead_lines=1, gap=(30, 34)))
    plain = D.generate(vol, cfg, str(root / "plain"), "phantom", n_train=20, n_test=4, seed=0)
    w = np.load(os.path.join(masked, "weights_train.npy"))
    assert w.shape == (64, 64) and not w[:, 30:34].any() and 64 * 4 < int((w == 0).sum()) <= 64 * 4 + 41 + 64
    for e in json.load(open(os.path.join(masked, "meta_data.json")))["proj_train"]:
        assert not np.load(os.path.join(masked, e["file_path"]))[w == 0].any()      # the masked pixels are written as 0
    assert "weights_train" not in json.load(open(os.path.join(plain, "meta_data.json")))
    return dict(masked=masked, plain=plain, nan=_copy_case(masked, str(root / "nan" / "phantom_cone"), fill=np.nan),
                ones=_copy_case(plain, str(root / "ones" / "phantom_cone"), weights=np.ones((64, 64))), root=root)


def _train(case, out, *extra):
    return subprocess.run([sys.executable, "-m", "r2_gaussian_amd.train", "-s", case, "-m", out] + COMMON + list(extra), cwd=ROOT,
                          capture_output=True, text=True, timeout=600)


def _model(out):
    with open(os.path.join(out, "point_cloud", "iteration_%d" % ITERS, "point_cloud.pickle"), "rb") as f:
        d = pickle.load(f)
    return {k: np.asarray(d[k], np.float32) for k in ("xyz", "density", "scale", "rotation")}


def _same_bits(a, b):
    return all(a[k].shape == b[k].shape and np.array_equal(a[k].view(np.int32), b[k].view(np.int32)) for k in a)


def test_unmeasured_pixels_may_hold_anything(cases):
    outs = {}
    for name in ("masked", "nan"):
        out = str(cases["root"] / ("out_" + name))
        r = _train(cases[name], out)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-5000:]
        outs[name] = _model(out)
    assert all(np.isfinite(v).all() for v in outs["masked"].values()) and outs["masked"]["xyz"].shape[0] > 0
    assert _same_bits(outs["masked"], outs["nan"])
    assert np.isfinite(np.load(os.path.join(str(cases["root"] / "out_nan"), "point_cloud", "iteration_%d" % ITERS, "vol_pred.npy"))).all()


def test_unit_weights_train_to_the_bits_of_no_weights(cases):
    models = []
    for k, extra in enumerate(((), ("--loss_weights", "none"))):
        out = str(cases["root"] / ("out_ones_%d" % k))
        r = _train(cases["ones"], out, *extra)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-5000:]
        models.append(_model(out))
    assert all(np.isfinite(v).all() for v in models[0].values())
    assert _same_bits(models[0], models[1])


def test_file_mode_needs_recorded_weights(cases):
    out = str(cases["root"] / "out_file")
    r = _train(cases["plain"], out, "--loss_weights", "file")
    assert r.returncode != 0 and "usage:" in r.stderr and "--loss_weights file" in r.stderr
    assert not os.path.exists(os.path.join(out, "point_cloud"))


def test_views_per_step_with_weights(cases):
    import yaml
    out = str(cases["root"] / "out_w4")
    r = _train(cases["nan"], out, "--views_per_step", "4", "--save_uncertainty", "1.0")
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-5000:]
    m = _model(out)
    assert all(np.isfinite(v).all() for v in m.values()) and m["xyz"].shape[0] > 0
    e = yaml.safe_load(open(os.path.join(out, "eval", "iter_%06d" % ITERS, "eval3d.yml")))
    assert np.isfinite(e["psnr_3d"])
    pc = os.path.join(out, "point_cloud", "iteration_%d" % ITERS)
    assert np.isfinite(np.load(os.path.join(pc, "vol_std.npy"))).all()
    assert all(np.isfinite(v).all() for v in np.load(os.path.join(pc, "fisher.npz")).values())
