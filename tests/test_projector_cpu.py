"""The volume forward projector on the CPU: the float64 restatement (tests/projector_ref.py) against analytic line
integrals, the product's host-side ray parameters against the restatement's, the training-noise restatement, and the dataset
writer's on-disk layout read back through a restatement of the reference reader (dataset_readers.py:43-76, 94-145)."""
import json
import os

import numpy as np
import pytest

from r2_gaussian_amd import datagen as D
from r2_gaussian_amd import projector as K
from r2_gaussian_amd import scene as S
from tests import projector_ref as PR


def blob_volume(n, sVoxel, center, c0, sigma, rho):
    """rho exp(-|x - c0|^2 / 2 sigma^2) sampled at the voxel centres center - sVoxel/2 + (i + 1/2) dVoxel."""
    axes = [center[a] - sVoxel[a] / 2 + (np.arange(n[a]) + 0.5) * sVoxel[a] / n[a] for a in range(3)]
    X, Y, Z = np.meshgrid(*axes, indexing="ij")
    r2 = (X - c0[0]) ** 2 + (Y - c0[1]) ** 2 + (Z - c0[2]) ** 2
    return rho * np.exp(-r2 / (2 * sigma * sigma))


def blob_line_integrals(view, H, W, c0, sigma, rho):
    """rho sqrt(2 pi) sigma exp(-b^2 / 2 sigma^2) for the ray of every pixel (b: distance of c0 from the ray), in world
    units, rays straight from the camera definition (not from the ray parameters)."""
    C2W = np.linalg.inv(view.world_view_transform.double().numpy().T)
    c = ((np.arange(W) + 0.5) * 2.0 / W - 1.0)
    r = ((np.arange(H) + 0.5) * 2.0 / H - 1.0)
    R, Cc = np.meshgrid(r, c, indexing="ij")
    if view.mode == 1:
        dv = np.stack([Cc * view.tanfovx, R * view.tanfovy, np.ones_like(R)], -1)
        org = np.broadcast_to(C2W[:3, 3], dv.shape)
    else:
        dv = np.broadcast_to(np.array([0.0, 0.0, 1.0]), R.shape + (3,))
        org = np.stack([Cc, R, np.zeros_like(R)], -1) @ C2W[:3, :3].T + C2W[:3, 3]
    d = dv @ C2W[:3, :3].T
    d = d / np.linalg.norm(d, axis=-1, keepdims=True)
    w = np.asarray(c0) - org
    b2 = (w * w).sum(-1) - (w * d).sum(-1) ** 2
    return rho * np.sqrt(2 * np.pi) * sigma * np.exp(-b2 / (2 * sigma * sigma))


CASES = {
    "cone_iso": dict(mode="cone", sVoxel=(2.0, 2.0, 2.0), center=(0.0, 0.0, 0.0), shape=(1, 1, 1), c0=(0.1, -0.05, 0.08)),
    "parallel_iso": dict(mode="parallel", sVoxel=(2.0, 2.0, 2.0), center=(0.0, 0.0, 0.0), shape=(1, 1, 1), c0=(0.1, -0.05, 0.08)),
    "cone_aniso_off": dict(mode="cone", sVoxel=(1.8, 1.5, 2.1), center=(0.12, -0.07, 0.05), shape=(1.0, 0.75, 1.25),
                           c0=(0.2, -0.1, 0.1)),
    "parallel_aniso_off": dict(mode="parallel", sVoxel=(1.8, 1.5, 2.1), center=(0.12, -0.07, 0.05), shape=(1.0, 0.75, 1.25),
                               c0=(0.2, -0.1, 0.1)),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_converges_to_analytic_line_integrals(name):
    cs = CASES[name]
    scanner = S.CONE_BEAM if cs["mode"] == "cone" else S.PARALLEL_BEAM
    H, W, sigma, rho = 18, 22, 0.16, 1.3
    views = [S.make_view(a, (H, W), scanner) for a in (0.3, 1.9, 4.4)]
    truth = np.stack([blob_line_integrals(v, H, W, cs["c0"], sigma, rho) for v in views])
    errs = []
    for base in (24, 48, 96):
        n = tuple(max(1, int(round(base * f))) for f in cs["shape"])
        vol = blob_volume(n, cs["sVoxel"], cs["center"], cs["c0"], sigma, rho)
        rays = PR.rays(views, cs["sVoxel"], cs["center"], n)
        dvox = np.array(cs["sVoxel"]) / np.array(n)
        got = PR.project(vol, rays, cs["mode"] == "cone", dvox, 0.5, H, W)["value"].reshape(len(views), H, W)
        errs.append(np.abs(got - truth).max() / truth.max())
    # h^2: halving the voxel size quarters the error (interpolation and midpoint rule are both second order); the coarsest
    # grid (4 voxels per sigma) is not quite asymptotic yet.  Measured ratios 2.9-4.1 and 4.0-4.6 per halving.
    assert errs[0] / errs[1] > 2.5 and errs[1] / errs[2] > 3.5 and errs[0] / errs[2] > 12.0, errs
    assert errs[2] < 4e-3, errs


def test_product_ray_parameters_are_the_restatements():
    for scanner, angles in ((S.CONE_BEAM, (0.0, np.pi / 4, 2.5)), (S.PARALLEL_BEAM, (0.0, np.pi / 2, 5.1))):
        views = [S.make_view(a, (30, 44), scanner) for a in angles]
        args = ((1.8, 1.5, 2.1), (0.12, -0.07, 0.05), (20, 17, 23))
        got = K.ray_params(views, *args)
        want = PR.rays(views, *args)
        assert got.dtype == np.float32 and got.shape == (3, 12)
        assert np.abs(got - want).max() <= 2.0 ** -23 * np.abs(want).max() * 4


def test_cone_ray_through_the_centre_pixel_hits_the_origin_voxel():
    """The ray of the detector's centre (odd sizes) runs from the source through the volume centre."""
    v = S.make_view(0.7, (33, 33), S.CONE_BEAM)
    r = PR.rays([v], (2.0, 2.0, 2.0), (0.0, 0.0, 0.0), (16, 16, 16))[0]
    P = r[3:6] + 16 * r[6:9] + 16 * r[9:12]
    d = P - r[0:3]
    t = np.dot(np.array([7.5, 7.5, 7.5]) - r[0:3], d) / np.dot(d, d)
    assert np.linalg.norm(r[0:3] + t * d - 7.5) < 1e-9


# ------------------------------------------------------------------------------------------------------------------- noise
NOISE_CFG = dict(noise=True, possion_noise=10000, gaussian_noise=[0, 10])


def test_noise_is_reproducible_for_a_seed():
    p = np.random.RandomState(1).rand(3, 8, 9).astype(np.float32) * 2.0
    a = D.noisy_train(p, NOISE_CFG, np.random.RandomState(7))
    b = D.noisy_train(p, NOISE_CFG, np.random.RandomState(7))
    c = D.noisy_train(p, NOISE_CFG, np.random.RandomState(8))
    assert a.dtype == np.float32 and a.shape == p.shape
    assert np.array_equal(a, b) and not np.array_equal(a, c)
    assert (a >= 0).all()


def test_noise_off_is_the_identity():
    p = np.random.RandomState(1).rand(3, 8, 9).astype(np.float32)
    rng = np.random.RandomState(7)
    state = rng.get_state()[1].copy()
    assert D.noisy_train(p, dict(NOISE_CFG, noise=False), rng) is p
    assert np.array_equal(rng.get_state()[1], state)   # and draws nothing


def test_noise_statistics():
    """-log(I / I0) m with I ~ Poisson(I0 e^(-p/m)) + N(0, sigma): mean p (to first order), variance
    m^2 (lam + sigma^2) / lam^2 with lam = I0 e^(-p/m) (delta method)."""
    m, i0, sigma = 3.0, 10000.0, 10.0
    levels = np.array([m, m / 2, m / 8])
    p = np.repeat(levels[:, None], 200000, 1).astype(np.float32)
    out = D.add_noise(p, i0, [0.0, sigma], np.random.RandomState(3)).astype(np.float64)
    lam = i0 * np.exp(-levels / m)
    sd = m * np.sqrt(lam + sigma ** 2) / lam
    assert np.all(np.abs(out.mean(1) - levels) < 4 * sd / np.sqrt(p.shape[1]) + 0.5 * sd ** 2 / m), (out.mean(1), levels)
    assert np.all(np.abs(out.std(1) / sd - 1.0) < 0.02), (out.std(1), sd)
    # the clip: a zero projection stays >= 0 and is zero about half the time
    z = D.add_noise(np.concatenate([p[:1, :10], np.zeros((1, 100000), np.float32)], 1), i0, [0.0, sigma],
                    np.random.RandomState(4))
    assert (z >= 0).all() and 0.4 < (z[0, 10:] == 0).mean() < 0.6


def test_angles_follow_the_reference():
    cfg = dict(totalAngle=180.0, startAngle=10.0)
    tr, te = D.angles_for(cfg, 6, 5, np.random.RandomState(2))
    assert np.allclose(tr, np.linspace(0, np.pi, 7)[:-1] + np.pi / 18)
    want = np.sort(np.random.RandomState(2).rand(5) * 2 * np.pi) + np.pi / 18
    assert np.array_equal(te, want)


# ---------------------------------------------------------------------------------------------------- dataset layout
def read_case(path):
    """Restatement of the reference reader's few lines that touch the files (dataset_readers.py:43-76, 94-145): the
    scanner's derived sizes, scene_scale, the per-frame image (np.load(...) * scene_scale), angle and detector size."""
    with open(os.path.join(path, "meta_data.json"), "r") as f:
        meta = json.load(f)
    meta["vol"] = os.path.join(path, meta["vol"])
    sc = meta["scanner"]
    sc.setdefault("dVoxel", list(np.array(sc["sVoxel"]) / np.array(sc["nVoxel"])))
    sc.setdefault("dDetector", list(np.array(sc["sDetector"]) / np.array(sc["nDetector"])))
    scale = 2 / max(sc["sVoxel"])
    for k in ("dVoxel", "sVoxel", "sDetector", "dDetector", "offOrigin", "offDetector", "DSD", "DSO"):
        sc[k] = (np.array(sc[k]) * scale).tolist()
    frames = {}
    for split in ("train", "test"):
        frames[split] = []
        for info in meta["proj_" + split]:
            image = np.load(os.path.join(path, info["file_path"])) * scale
            frames[split].append(dict(angle=info["angle"], image=image, width=sc["nDetector"][1],
                                      height=sc["nDetector"][0], name=os.path.basename(info["file_path"]).split(".")[0]))
    vol = np.load(meta["vol"])
    return meta, frames, vol, scale


def test_dataset_layout_reads_back(tmp_path):
    import yaml
    with open(os.path.join(os.path.dirname(__file__), "golden", "scanner", "cone_beam.yml")) as f:
        cfg = yaml.safe_load(f)
    cfg = dict(cfg, nDetector=[6, 7], nVoxel=[4, 5, 3], sVoxel=[2.0, 2.0, 1.0])
    rng = np.random.RandomState(0)
    vol = rng.rand(4, 5, 3).astype(np.float32)
    tr_a, te_a = D.angles_for(cfg, 4, 3, rng)
    tr = rng.rand(4, 6, 7).astype(np.float32)
    te = rng.rand(3, 6, 7).astype(np.float32)
    case = os.path.join(str(tmp_path), "phantom_cone")
    D.write_case(case, cfg, vol, tr, tr_a, te, te_a)
    assert sorted(os.listdir(case)) == ["meta_data.json", "proj_test", "proj_train", "vol_gt.npy"]
    assert sorted(os.listdir(os.path.join(case, "proj_train"))) == ["proj_train_%04d.npy" % i for i in range(4)]
    assert sorted(os.listdir(os.path.join(case, "proj_test"))) == ["proj_test_%04d.npy" % i for i in range(3)]
    raw = json.load(open(os.path.join(case, "meta_data.json")))
    assert sorted(raw) == ["bbox", "proj_test", "proj_train", "scanner", "vol"]
    assert raw["vol"] == "vol_gt.npy" and raw["bbox"] == [[-1, -1, -1], [1, 1, 1]] and raw["scanner"] == cfg
    for e in raw["proj_train"] + raw["proj_test"]:
        assert sorted(e) == ["angle", "file_path"] and isinstance(e["angle"], float) and isinstance(e["file_path"], str)
    meta, frames, vol_back, scale = read_case(case)
    assert scale == 1.0 and np.array_equal(vol_back, vol) and vol_back.dtype == np.float32
    for split, stack, angles in (("train", tr, tr_a), ("test", te, te_a)):
        assert len(frames[split]) == len(stack)
        for i, fr in enumerate(frames[split]):
            raw_img = np.load(os.path.join(case, "proj_%s" % split, "proj_%s_%04d.npy" % (split, i)))
            assert raw_img.dtype == np.float32 and raw_img.shape == (fr["height"], fr["width"]) == (6, 7)
            assert np.array_equal(fr["image"], stack[i]) and fr["angle"] == float(angles[i])
            assert fr["name"] == "proj_%s_%04d" % (split, i)


def test_input_validation_on_the_host():
    cfg = dict(S.CONE_BEAM, nVoxel=[4, 4, 4])
    with pytest.raises(ValueError):
        K.project(np.zeros((4, 4), np.float32), [0.0], cfg)
    with pytest.raises(ValueError):
        K.project(np.zeros((4, 4, 5), np.float32), [0.0], cfg)
    with pytest.raises(ValueError):
        K.project(np.zeros((4, 4, 4), np.float32), [0.0], cfg, accuracy=0.0)
    from r2_gaussian_amd._lib import R2HipError
    import torch
    with pytest.raises(R2HipError):
        K.project_views(torch.zeros(4, 4, 4), [S.make_view(0.0, (8, 8))], (2, 2, 2), (0, 0, 0))   # CPU tensor: no fallback
