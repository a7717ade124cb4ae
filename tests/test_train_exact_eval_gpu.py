"""GPU: ``--eval_exact`` of the native trainer writes eval2d_render_{train,test}_exact.yml (finite values, the usual keys) at
every evaluation; without the flag the set of files is what it was."""
import math
import os

import numpy as np
import pytest
import yaml

pytestmark = pytest.mark.gpu


def _files(root):
    return sorted(os.path.relpath(os.path.join(dp, f), root) for dp, _, fs in os.walk(root) for f in fs)


def test_eval_exact_adds_two_files_per_evaluation(gpu, tmp_path):
    from r2_gaussian_amd import datagen as D
    from r2_gaussian_amd import scene as S
    from r2_gaussian_amd import train as TR
    n = 32
    ax = -1 + (np.arange(n) + 0.5) * 2.0 / n
    X, Y, Z = np.meshgrid(ax, ax, ax, indexing="ij")
    vol = (0.6 * np.exp(-((X - 0.1) ** 2 + (Y + 0.2) ** 2 + Z ** 2) / (2 * 0.3 ** 2))).astype(np.float32)
    cfg = dict(S.CONE_BEAM, nVoxel=[n, n, n], nDetector=[32, 32], noise=False, totalAngle=360.0, startAngle=0.0)
    case = D.generate(vol, cfg, str(tmp_path / "data"), "blob", n_train=6, n_test=3, seed=0)
    common = ["-s", case, "--iterations", "30", "--test_iterations", "30", "--quiet"]
    TR.main(common + ["-m", str(tmp_path / "plain")])
    TR.main(common + ["-m", str(tmp_path / "exact"), "--eval_exact"])
    plain, exact = _files(str(tmp_path / "plain")), _files(str(tmp_path / "exact"))
    extra = sorted(set(exact) - set(plain))
    assert set(plain) <= set(exact)
    assert extra == sorted(os.path.join("eval", "iter_%06d" % it, "eval2d_render_%s_exact.yml" % s) for it in (1, 30)
                           for s in ("train", "test"))
    assert not any("exact" in f for f in plain)
    for f in extra:
        e = yaml.safe_load(open(os.path.join(str(tmp_path / "exact"), f)))
        assert list(e) == ["psnr_2d", "ssim_2d", "psnr_2d_projs", "ssim_2d_projs"]
        assert math.isfinite(e["psnr_2d"]) and math.isfinite(e["ssim_2d"])
        assert len(e["psnr_2d_projs"]) == (6 if "train" in f else 3) and all(math.isfinite(x) for x in e["psnr_2d_projs"])
    # the exact projection of a model that fits the data is close to the rasterizer's image of it
    a = yaml.safe_load(open(os.path.join(str(tmp_path / "exact"), "eval", "iter_000030", "eval2d_render_test.yml")))
    b = yaml.safe_load(open(os.path.join(str(tmp_path / "exact"), "eval", "iter_000030", "eval2d_render_test_exact.yml")))
    print("psnr_2d rasterizer %.3f, exact %.3f" % (a["psnr_2d"], b["psnr_2d"]))
