"""The Siddon projector on the CPU: the float64 restatement (tests/siddon_ref.py) against analytic ray/box chords, a single
voxel, the rows of its dense matrix, its convergence towards the interpolated model on a smooth volume, and the host-side
validation of ``projection_type``."""
import json
import os

import numpy as np
import pytest

from r2_gaussian_amd import datagen as D
from r2_gaussian_amd import projector as K
from r2_gaussian_amd import recon as RC
from r2_gaussian_amd import scene as S
from tests import projector_ref as PR
from tests import siddon_ref as SR
from tests.test_projector_cpu import blob_volume

GEOMS = {
    # name: scanner, (H, W), nVoxel, sVoxel, center, angles
    "cone_aniso_offset": (S.CONE_BEAM, (11, 13), (9, 7, 8), (1.8, 1.4, 1.7), (0.1, -0.05, 0.07), (0.3, 2.1, 4.0)),
    "parallel_aniso_offset": (S.PARALLEL_BEAM, (11, 13), (9, 7, 8), (1.8, 1.4, 1.7), (0.1, -0.05, 0.07), (0.3, 2.1, 4.0)),
    "cone_misses": (S.CONE_BEAM, (11, 13), (9, 7, 8), (0.6, 0.7, 0.5), (0.35, -0.3, 0.2), (0.2, 2.0, 4.1)),
    "parallel_misses": (S.PARALLEL_BEAM, (11, 13), (9, 7, 8), (0.6, 0.7, 0.5), (0.35, -0.3, 0.2), (0.2, 2.0, 4.1)),
}


def _slab_chord(S0, D0, lo, hi, cone):
    """Length in t of the line S0 + t D0 inside the box [lo, hi] (t >= 0 for a cone ray): the slab method, vectorised."""
    with np.errstate(divide="ignore", invalid="ignore"):
        ta, tb = (lo - S0) / D0, (hi - S0) / D0
    t0 = np.where(D0 != 0, np.minimum(ta, tb), -np.inf).max(1)
    t1 = np.where(D0 != 0, np.maximum(ta, tb), np.inf).min(1)
    ok = ((D0 != 0) | ((S0 >= lo) & (S0 < hi))).all(1)
    if cone:
        t0 = np.maximum(t0, 0.0)
    return np.where(ok, np.maximum(t1 - t0, 0.0), 0.0)


def _setup(name):
    scanner, det, n, s, ctr, angles = GEOMS[name]
    views = [S.make_view(a, det, scanner) for a in angles]
    rays32 = K.ray_params(views, s, ctr, n)
    dvox = np.asarray(s, np.float64) / np.asarray(n)
    return views, rays32, dvox, views[0].mode == 1, det, n, s, ctr


@pytest.mark.parametrize("name", sorted(GEOMS))
def test_constant_volume_is_the_chord_length(name):
    """A volume of ones integrates to the world length of the ray inside the volume's box: the slab method in world
    coordinates on the same float32 ray parameters, to float64 rounding."""
    views, rays32, dvox, cone, (H, W), n, s, ctr = _setup(name)
    got = SR.project(np.ones(n), rays32, cone, dvox, H, W)
    S0, D0, _, _ = SR._ray_geometry(rays32, cone, got["pixels"])
    corner = np.asarray(ctr, np.float64) - 0.5 * np.asarray(s, np.float64)
    Sw, Dw = corner + (S0 + 0.5) * dvox, D0 * dvox                    # index -> world
    want = _slab_chord(Sw, Dw, corner, corner + np.asarray(s, np.float64), cone) * np.sqrt((Dw * Dw).sum(1))
    assert (want > 0).sum() >= 20
    if "misses" in name:
        assert (want == 0).sum() > 0.2 * len(want)
    assert np.abs(got["value"] - want).max() <= 1e-12 * want.max()
    assert np.abs(got["chord"] - want).max() <= 1e-12 * want.max()
    assert ((got["value"] > 0) == got["hit"]).all()


@pytest.mark.parametrize("name", ["cone_aniso_offset", "parallel_aniso_offset"])
def test_single_voxel_is_the_ray_cube_length(name):
    views, rays32, dvox, cone, (H, W), n, s, ctr = _setup(name)
    for v in ((4, 3, 4), (0, 0, 0), (8, 6, 7), (2, 5, 1)):
        vol = np.zeros(n)
        vol[v] = 1.0
        got = SR.project(vol, rays32, cone, dvox, H, W)
        S0, D0, _, _ = SR._ray_geometry(rays32, cone, got["pixels"])
        c = np.asarray(v, np.float64)
        want = _slab_chord(S0, D0, c - 0.5, c + 0.5, cone) * np.sqrt(((D0 * dvox) ** 2).sum(1))
        assert (want > 0).any()
        assert np.abs(got["value"] - want).max() <= 1e-12 * max(dvox)


@pytest.mark.parametrize("name", sorted(GEOMS))
def test_dense_rows_sum_to_the_chords(name):
    views, rays32, dvox, cone, (H, W), n, s, ctr = _setup(name)
    A = SR.dense_A(views, s, ctr, n)
    ref = SR.project(np.ones(n), rays32, cone, dvox, H, W)
    assert A.shape == (len(views) * H * W, int(np.prod(n))) and (A >= 0).all()
    assert np.abs(A.sum(1) - ref["chord"]).max() <= 1e-12 * ref["chord"].max()
    # and A applied to a volume is the projection of that volume
    x = np.random.RandomState(3).rand(*n)
    assert np.abs(A @ x.ravel() - SR.project(x, rays32, cone, dvox, H, W)["value"]).max() <= 1e-12 * ref["chord"].max()


@pytest.mark.parametrize("mode", ["cone", "parallel"])
def test_converges_towards_the_interpolated_model(mode):
    """On a smooth blob the two models differ to first order in the voxel size: the piecewise-constant volume takes the value
    of the nearest voxel centre, up to half a voxel off the ray across it, where the interpolated one is second order.  The
    difference therefore halves with the voxel size: it must shrink at every halving, and by more than 2.5 over two of them
    (first order gives 4)."""
    scanner = S.CONE_BEAM if mode == "cone" else S.PARALLEL_BEAM
    H, W, sigma, rho = 7, 8, 0.2, 1.3
    sV, ctr, c0 = (1.8, 1.5, 2.1), (0.12, -0.07, 0.05), (0.2, -0.1, 0.1)
    views = [S.make_view(a, (H, W), scanner) for a in (0.3, 1.9)]
    errs = []
    for base in (12, 24, 48):
        n = (base, base, base)
        vol = blob_volume(n, sV, ctr, c0, sigma, rho)
        rays32 = K.ray_params(views, sV, ctr, n)
        dvox = np.array(sV) / np.array(n)
        sid = SR.project(vol, rays32, mode == "cone", dvox, H, W)["value"]
        itp = PR.project(vol, rays32, mode == "cone", dvox, 0.125, H, W)["value"]
        errs.append(np.abs(sid - itp).max() / itp.max())
    assert errs[0] > errs[1] > errs[2] and errs[0] / errs[2] > 2.5, errs


def test_exact_ties_and_flat_axes():
    """Hand-made parallel rays along (1, 1, 0) through lattice-symmetric points: every x crossing ties with a y crossing and
    the z axis is flat.  The chord through the 4^3 unit volume is 4 sqrt(2) for the rays through the diagonal."""
    rays = np.array([[1.0, 1.0, 0.0, -2.0, -2.0, -0.25, 1.0, -1.0, 0.0, 0.0, 0.0, 0.5]], np.float32)
    got = SR.project(np.ones((4, 4, 4)), rays, False, (1.0, 1.0, 1.0), 9, 1)
    want = np.where(np.arange(9) < 8, 4 * np.sqrt(2.0), 0.0)      # z = -0.25 + r / 2: the ninth row is outside
    assert np.abs(got["value"] - want).max() <= 1e-12
    A = SR.dense_A_rays(rays, False, (1.0, 1.0, 1.0), (4, 4, 4), 9, 1)
    diag = np.zeros((4, 4, 4))
    diag[np.arange(4), np.arange(4), 1] = np.sqrt(2.0)
    assert np.abs(A[3].reshape(4, 4, 4) - diag).max() <= 1e-12     # row 3: z = 1.25, slab 1


def test_projection_type_is_validated_on_the_host(tmp_path):
    cfg = dict(S.CONE_BEAM, nVoxel=[4, 4, 4], nDetector=[6, 7])
    vol = np.zeros((4, 4, 4), np.float32)
    views = [S.make_view(0.0, (6, 7))]
    import torch
    for bad in ("Siddon", "ray-voxel", "", None, 1):
        with pytest.raises(ValueError):
            K.project(vol, [0.0], cfg, projection_type=bad)
        with pytest.raises(ValueError):
            K.project_views(torch.zeros(4, 4, 4), views, (2, 2, 2), (0, 0, 0), projection_type=bad)
        with pytest.raises(ValueError):
            RC.backproject_views(torch.zeros(1, 6, 7), views, (2, 2, 2), (0, 0, 0), nVoxel=(4, 4, 4), projection_type=bad)
        with pytest.raises(ValueError):
            RC.Operator([0.0], cfg, projection_type=bad)
        with pytest.raises(ValueError):
            RC.reconstruct(np.zeros((1, 6, 7), np.float32), [0.0], cfg, "cgls", projection_type=bad)
    with pytest.raises(ValueError):
        D.generate(vol, cfg, str(tmp_path), "x", 2, 1, projection_type="nearest")
    with pytest.raises(SystemExit):
        D.main(["--projection_type", "nearest"])
    with pytest.raises(SystemExit):
        RC.main(["-s", "a", "-m", "b", "--projection_type", "nearest"])
    assert not os.listdir(str(tmp_path))
    # accuracy is not looked at for "siddon": the type check comes first, then the GPU requirement
    from r2_gaussian_amd._lib import R2HipError
    with pytest.raises(R2HipError):
        K.project_views(torch.zeros(4, 4, 4), views, (2, 2, 2), (0, 0, 0), accuracy=0.0, projection_type="siddon")


def test_a_case_records_its_projection_type(tmp_path):
    cfg = dict(S.CONE_BEAM, nVoxel=[4, 5, 3], nDetector=[6, 7])
    rng = np.random.RandomState(0)
    args = (rng.rand(4, 5, 3), rng.rand(2, 6, 7), [0.0, 1.0], rng.rand(1, 6, 7), [0.5])
    D.write_case(str(tmp_path / "a"), dict(cfg, projection_type="siddon"), *args)
    D.write_case(str(tmp_path / "b"), cfg, *args)
    rec = {k: json.load(open(os.path.join(str(tmp_path / k), "meta_data.json")))["scanner"] for k in "ab"}
    assert D.recorded_projection_type(rec["a"]) == "siddon" and rec["a"]["projection_type"] == "siddon"
    assert D.recorded_projection_type(rec["b"]) == "interpolated" and rec["b"] == cfg
    assert D.recorded_projection_type(RC._read_case(str(tmp_path / "a"))["cfg"]) == "siddon"
    with pytest.raises(ValueError):
        D.recorded_projection_type(dict(cfg, projection_type="nearest"))


def test_the_binding_holds_both_symbols():
    from r2_gaussian_amd import _lib
    syms = _lib.exported_symbols()
    assert "r2_project_volume_siddon" in syms and "r2_backproject_volume_siddon" in syms
    fwd, bwd = _lib._SIGNATURES["r2_project_volume_siddon"], _lib._SIGNATURES["r2_backproject_volume_siddon"]
    # r2_project_volume's arguments without `accuracy`
    want = list(_lib._SIGNATURES["r2_project_volume"][1])
    del want[11]
    assert fwd[1] == want and bwd[1] == want
    L = _lib.lib()
    assert hasattr(L, "r2_project_volume_siddon") and hasattr(L, "r2_backproject_volume_siddon")
