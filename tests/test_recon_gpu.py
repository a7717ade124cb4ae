"""The exact adjoint of the projector (csrc/backprojector.hip), the TV descent (csrc/tv_descent.hip) and the iterative
reconstructions on top of them (r2_gaussian_amd/recon.py) on the MI355X: the transpose entry by entry, the dot test, the
algorithms against their float64 restatement (tests/recon_ref.py), identities, a physical anchor, the CLI end to end, no
host synchronisation inside the iterations, and validation."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from r2_gaussian_amd import datagen as D
from r2_gaussian_amd import fdk as F
from r2_gaussian_amd import projector as K
from r2_gaussian_amd import recon as RC
from r2_gaussian_amd import scene as S
from tests import helpers as Hh
from tests import projector_ref as PR
from tests import recon_ref as RR
from tests.operator_cases import TINY_ANGLES, TRANSPOSE, _tiny_cfg, one_hot_matrices, tiny_system

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24


@pytest.mark.parametrize("case", TRANSPOSE, ids=[c[0] for c in TRANSPOSE])
def test_transpose_entry_by_entry(gpu, case):
    """A from one-hot volumes through the projector, A^T from one-hot pixels through the back-projector: the same zero
    pattern exactly, and every entry within (2 n + 8) u |entry| (n: the ray's sample count; per side a product of three
    weights, a sum of at most n sample terms and two scalings)."""
    name, scanner, det, n, s, ctr, angles, acc = case
    views = [S.make_view(a, det, scanner) for a in angles]
    fwd, bwd = (m.astype(np.float64) for m in one_hot_matrices(gpu, views, det, n, s, ctr, acc))   # exact widening
    assert np.array_equal(fwd == 0, bwd == 0), (name, int(((fwd == 0) != (bwd == 0)).sum()))
    rays32 = K.ray_params(views, s, ctr, n)
    ref = PR.project(np.zeros(n), rays32, views[0].mode == 1, np.asarray(s) / np.asarray(n), acc, *det)
    nray = np.maximum(ref["n_hi"], ref["n"]).astype(np.float64)[:, None]
    bound = (2 * nray + 8) * U * np.maximum(np.abs(fwd), np.abs(bwd))
    err = np.abs(fwd - bwd)
    assert (err <= bound).all(), (name, float((err / np.maximum(bound, 1e-300)).max()))
    st = {"nonzero": int((fwd != 0).sum()), "max_err_over_bound": float((err / np.maximum(bound, 1e-300)).max()),
          "rays_missing": int((fwd == 0).all(1).sum()), "rays": int(fwd.shape[0])}
    Hh._log("recon", "transpose " + name, lambda: st)
    assert st["nonzero"] > 0
    if "misses" in name:
        assert st["rays_missing"] > 0.2 * st["rays"]


def test_dot_test_128(gpu):
    """<A x, y> = <x, A^T y> at 128^3 <- 32 x 128^2 (cone, offset, anisotropic), within (n_max + P + V + 8) u sum |terms|:
    n_max samples per ray, P <= 64 pixels per voxel and view in the gather's box at this scanner, V views."""
    g = torch.Generator(device=gpu).manual_seed(0)
    n, det, V = (128, 128, 128), (128, 128), 32
    views = [S.make_view(a, det, S.CONE_BEAM) for a in np.linspace(0, 2 * np.pi, V + 1)[:-1] + 0.1]
    s, ctr = (2.0, 1.8, 2.1), (0.05, -0.02, 0.03)
    x = torch.rand(n, device=gpu, generator=g)
    y = torch.rand((V,) + det, device=gpu, generator=g)
    Ax = K.project_views(x, views, s, ctr, 0.5)
    Aty = RC.backproject_views(y, views, s, ctr, 0.5, nVoxel=n)
    lhs = float((Ax.double() * y.double()).sum())
    rhs = float((x.double() * Aty.double()).sum())
    terms = lhs   # x, y >= 0 and A >= 0: sum |terms| = <A x, y>
    n_max = np.ceil(np.sqrt(sum(m ** 2 for m in n)) / 0.5) + 8
    bound = (n_max + 64 + V + 8) * U * terms
    st = {"rel_diff": abs(lhs - rhs) / terms, "bound_rel": bound / terms}
    Hh._log("recon", "dot test 128^3 <- 32 x 128^2", lambda: st)
    assert abs(lhs - rhs) <= bound, st


def _tiny_system(mode):
    cfg = _tiny_cfg(mode)
    A, bd = RR.dense_A_cfg(cfg, TINY_ANGLES)
    assert not bd.any(), "a ray of the tiny geometry sits on an n or hit/miss boundary: choose another"
    return cfg, A, tiny_system(cfg, A), tuple(cfg["nVoxel"])


def _rel(a, b):
    return float(np.abs(np.asarray(a, np.float64) - b).max() / max(np.abs(b).max(), 1e-30))


@pytest.mark.parametrize("mode", ["cone", "parallel"])
def test_cgls_first_iterates_match_the_restatement(gpu, mode):
    cfg, A, b, n = _tiny_system(mode)
    H, W = cfg["nDetector"]
    bt = torch.from_numpy(b.reshape(len(TINY_ANGLES), H, W)).to(gpu)
    xs, l2 = RR.cgls(A, b.astype(np.float64), 4)
    errs = []
    for k in range(1, 5):
        got = RC.cgls(bt, TINY_ANGLES, cfg, k).cpu().numpy().ravel()
        errs.append(_rel(got, xs[k - 1]))
    Hh._log("recon", "cgls vs float64 %s" % mode, lambda: {"rel_err_per_iterate": errs})
    assert max(errs) < 1e-4, errs


@pytest.mark.parametrize("mode", ["cone", "parallel"])
def test_sart_and_ossart_match_the_restatement(gpu, mode):
    cfg, A, b, n = _tiny_system(mode)
    H, W = cfg["nDetector"]
    bt = torch.from_numpy(b.reshape(len(TINY_ANGLES), H, W)).to(gpu)
    rows = H * W
    st = {}
    for bs in (1, 4):
        want = RR.ossart(A, b.astype(np.float64), rows, 2, bs, 1.0, 0.999)[-1]
        got = RC.ossart(bt, TINY_ANGLES, cfg, 2, bs).cpu().numpy().ravel()
        st["blocksize_%d" % bs] = _rel(got, want)
    Hh._log("recon", "ossart vs float64 %s" % mode, lambda: st)
    assert max(st.values()) < 1e-4, st


def test_asd_pocs_matches_the_restatement(gpu):
    cfg, A, b, n = _tiny_system("cone")
    H, W = cfg["nDetector"]
    bt = torch.from_numpy(b.reshape(len(TINY_ANGLES), H, W)).to(gpu)
    # maxl2err 0 and a long TV step: the dtvg reductions are decided by dg > rmax dp, and some of them are taken
    maxl2 = 0.0
    taken = 0
    for bs in (1, 3):
        x, tr = RC.os_asd_pocs(bt, TINY_ANGLES, cfg, 4, bs, tviter=5, maxl2err=maxl2, alpha=0.3, return_trace=True)
        dec = [bool(v) for v in tr["reduced"]]
        taken += sum(dec)
        want, rt = RR.os_asd_pocs(A, b.astype(np.float64), n, H * W, 4, bs, tviter=5, maxl2err=maxl2, alpha=0.3,
                                  decisions=dec)
        # the kernel's decisions are the restatement's own wherever they are not within float error of the threshold
        for it in range(len(rt["dg"])):
            own = rt["dg"][it] > 0.94 * rt["dp"][it] and rt["dd"][it] > maxl2
            clear = abs(rt["dg"][it] - 0.94 * rt["dp"][it]) > 1e-4 * rt["dg"][it] and abs(rt["dd"][it] - maxl2) > 1e-4 * maxl2
            assert own == dec[it] or not clear, (bs, it)
        assert all(bool(a) for a in tr["active"][:len(rt["dg"])])
        e = _rel(x.cpu().numpy().ravel(), want)
        Hh._log("recon", "os_asd_pocs vs float64 bs=%d" % bs, lambda: {"rel_err": e, "decisions": dec})
        assert e < 1e-3, e
    assert taken > 0


@pytest.mark.parametrize("shape", [(1, 1, 40), (1, 9, 13), (2, 2, 2), (37, 29, 53), (5, 1, 1)])
def test_tv_descent_matches_the_restatement(gpu, shape):
    rng = np.random.RandomState(sum(shape))
    x = rng.rand(*shape).astype(np.float32)
    got = RC.tv_descent(torch.from_numpy(x).to(gpu), 0.01 * np.sqrt(x.size), 5).cpu().numpy()
    want = RR.tv_descent(x, 0.01 * np.sqrt(x.size), 5)
    e = _rel(got, want)
    Hh._log("recon", "tv descent %s" % (shape,), lambda: {"rel_err": e})
    assert e < 1e-5, e
    assert RR.tv_value(got) < RR.tv_value(x)


def test_tv_descent_of_a_constant_volume(gpu):
    x = torch.full((6, 7, 8), 0.25, device=gpu)
    RC.tv_descent(x, 0.5, 3)
    assert bool(torch.isfinite(x).all()) and bool((x == 0.25).all())
    step = torch.full((), 0.5, device=gpu)   # a device step
    RC.tv_descent(x, step, 2)
    assert bool((x == 0.25).all())


def _blob(n, c0, sigma, rho):
    ax = -1 + (np.arange(n) + 0.5) * 2.0 / n
    X, Y, Z = np.meshgrid(ax, ax, ax, indexing="ij")
    return (rho * np.exp(-((X - c0[0]) ** 2 + (Y - c0[1]) ** 2 + (Z - c0[2]) ** 2) / (2 * sigma ** 2))).astype(np.float32)


def _phantom(n):
    return _blob(n, (0.1, -0.2, 0.05), 0.3, 0.6) + _blob(n, (-0.3, 0.25, -0.1), 0.12, 0.5) + _blob(n, (0.35, 0.3, 0.2), 0.08, 0.4)


def _cfg64(n=64, det=(96, 96), mode="cone"):
    base = S.CONE_BEAM if mode == "cone" else S.PARALLEL_BEAM
    return dict(base, nVoxel=[n, n, n], nDetector=list(det), accuracy=0.5, filter=None, noise=True, possion_noise=10000,
                gaussian_noise=[0, 10])


def test_identities(gpu):
    """Bit-reproducible back-projection, TV descent and CGLS; a NaN-filled out gives the same bits; OS-SART with one view per
    block is SART bit for bit; the CGLS residual does not increase; SART's and ASD-POCS's SART iterates are >= 0."""
    cfg = _cfg64(48, (64, 72))
    vol = _phantom(48)
    angles = np.linspace(0, 2 * np.pi, 21)[:-1]
    b = K.project(vol, angles, cfg)
    a1, a2 = RC.backproject(b, angles, cfg), RC.backproject(b, angles, cfg)
    assert torch.equal(a1, a2)
    op = RC.Operator(angles, cfg)
    out = torch.full(tuple(cfg["nVoxel"]), float("nan"), device=gpu)
    assert op.At(b, out=out) is out and torch.equal(out, a1)
    t1, t2 = a1.clone(), a1.clone()
    RC.tv_descent(t1, 0.3, 4)
    RC.tv_descent(t2, 0.3, 4)
    assert torch.equal(t1, t2) and not torch.equal(t1, a1)
    (c1, l2), c2 = RC.cgls(b, angles, cfg, 12, computel2=True), RC.cgls(b, angles, cfg, 12)
    assert torch.equal(c1, c2)
    # the recursive residual is float32: 1e-4 relative slack per step
    assert all(l2[i + 1] <= l2[i] * (1 + 1e-4) for i in range(len(l2) - 1)), l2
    s1 = RC.sart(b, angles, cfg, 3)
    s2 = RC.ossart(b, angles, cfg, 3, blocksize=1)
    assert torch.equal(s1, s2) and float(s1.min()) >= 0.0
    assert float(RC.ossart(b, angles, cfg, 2, blocksize=7).min()) >= 0.0
    _, tr = RC.asd_pocs(b, angles, cfg, 3, tviter=5, return_trace=True)
    assert all(float(m) >= 0.0 for m in tr["sart_min"])


# Physical anchor: 64^3 phantom, 60 noise-free cone views of 96^2.  First measurement on the MI355X: CGLS-20 66.65 dB,
# SART-10 71.44 dB (logged as "anchor" in the parity report); the thresholds sit at least 1 dB below them.
PSNR_MIN = {"cgls": 65.5, "sart": 70.0}


def test_physical_anchor(gpu):
    from r2_gaussian_amd.metrics import metric_vol
    cfg = _cfg64()
    vol = _phantom(64)
    angles = np.linspace(0, 2 * np.pi, 61)[:-1]
    b = K.project(vol, angles, cfg)
    got = {"cgls": RC.cgls(b, angles, cfg, 20), "sart": RC.sart(b, angles, cfg, 10)}
    psnr = {k: float(metric_vol(vol, v.cpu().numpy(), "psnr")[0]) for k, v in got.items()}
    # noisy projections: ASD-POCS ends with less TV than SART
    noisy = D.noisy_train(b.cpu().numpy(), cfg, np.random.RandomState(0))
    xs = RC.sart(noisy, angles, cfg, 10).cpu().numpy()
    xa = RC.asd_pocs(noisy, angles, cfg, 10).cpu().numpy()
    tv = {"sart": RR.tv_value(xs), "asd_pocs": RR.tv_value(xa)}
    Hh._log("recon", "anchor 64^3 <- 60 x 96^2", lambda: dict({"psnr_" + k: v for k, v in psnr.items()},
                                                              **{"tv_" + k: v for k, v in tv.items()}))
    print("anchor", psnr, tv)
    for k, v in psnr.items():
        assert v > PSNR_MIN[k], (k, v)
    assert tv["asd_pocs"] < tv["sart"], tv


def test_end_to_end_case_and_cli(gpu, tmp_path):
    vol = _phantom(32)
    cfg = dict(_cfg64(32, (40, 48)), noise=False, totalAngle=360.0, startAngle=0.0)
    case = D.generate(vol, cfg, str(tmp_path / "data"), "phantom", n_train=12, n_test=3, seed=1)
    rd = RC._read_case(case)
    projs, angles = rd["train"]
    v1 = F.recon_volume(projs, angles, cfg, "cgls")
    v2 = RC.cgls(projs, angles, cfg, 60).cpu().numpy()
    assert isinstance(v1, np.ndarray) and v1.shape == (32, 32, 32) and np.array_equal(v1, v2)
    out = str(tmp_path / "out")
    r = subprocess.run([sys.executable, "-m", "r2_gaussian_amd.recon", "-s", case, "-m", out, "--methods", "fdk", "sart",
                        "asd_pocs"], cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    import yaml
    top = yaml.safe_load(open(os.path.join(out, "eval_3d.yml")))
    keys = ["method", "psnr_3d", "ssim_3d", "ssim_3d_x", "ssim_3d_y", "ssim_3d_z", "duration (sec)", "duration (min)"]
    assert list(top) == ["fdk", "sart", "asd_pocs"]
    for m in top:
        assert list(top[m]) == keys and top[m]["method"] == m
        d = os.path.join(out, m)
        assert list(yaml.safe_load(open(os.path.join(d, "eval_3d.yml")))) == keys
        assert np.array_equal(np.load(os.path.join(d, "ct_gt.npy")), vol)
        assert np.load(os.path.join(d, "ct_pred.npy")).shape == (32, 32, 32)
        for i in range(32):
            for kind in ("gt", "pred"):
                assert os.path.exists(os.path.join(d, "slice_%s" % m, "%05d_%s.png" % (i, kind)))
        for i in range(3):
            for kind in ("render", "gt"):
                assert os.path.exists(os.path.join(d, "projs", "%05d_%s.npy" % (i, kind)))
                assert os.path.exists(os.path.join(d, "projs", "%05d_%s.png" % (i, kind)))
        assert np.load(os.path.join(d, "projs", "00000_render.npy")).shape == (40, 48)
    # the test-view renders are project() of the saved prediction, in the normalised scene's units like the gt files
    pred = np.load(os.path.join(out, "sart", "ct_pred.npy"))
    want = (K.project(pred, rd["test"][1], cfg) * rd["scale"]).cpu().numpy()
    assert np.array_equal(np.load(os.path.join(out, "sart", "projs", "00001_render.npy")), want[1])
    assert np.array_equal(np.load(os.path.join(out, "sart", "projs", "00001_gt.npy")), rd["test"][0][1] * np.float32(rd["scale"]))
    assert top["sart"]["psnr_3d"] > top["fdk"]["psnr_3d"] - 10.0


def test_no_host_sync_inside_the_iterations(gpu):
    cfg = _cfg64(32, (40, 48))
    angles = np.linspace(0, 2 * np.pi, 9)[:-1]
    b = K.project(_phantom(32), angles, cfg)
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        x = RC.cgls(b, angles, cfg, 5)
        y = RC.sart(b, angles, cfg, 2)
        z = RC.ossart(b, angles, cfg, 2, blocksize=3)
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    assert bool(torch.isfinite(x).all()) and bool(torch.isfinite(y).all()) and bool(torch.isfinite(z).all())


def test_validation_before_any_launch(gpu):
    from r2_gaussian_amd._lib import R2HipError
    views = [S.make_view(0.0, (8, 9))]
    out = torch.full((4, 5, 6), 7.0, device=gpu)
    p = torch.ones(1, 8, 9, device=gpu)
    for bad in (dict(projs=torch.ones(8, 9, device=gpu)), dict(projs=torch.ones(2, 8, 9, device=gpu)), dict(accuracy=0.0),
                dict(accuracy=float("nan")), dict(views=[]), dict(views=views + [S.make_view(0.1, (8, 10))]),
                dict(sVoxel=(2.0, -1.0, 2.0)), dict(out=torch.zeros(4, 5, 6, device=gpu, dtype=torch.float64)),
                dict(out=torch.zeros(6, 5, 4, device=gpu).transpose(0, 2)), dict(out=None)):
        kw = dict(projs=p, views=views, sVoxel=(2.0, 2.0, 2.0), center=(0.0, 0.0, 0.0), accuracy=0.5, out=out)
        kw.update(bad)
        with pytest.raises(ValueError):
            RC.backproject_views(**kw)
    with pytest.raises(R2HipError):
        RC.backproject_views(p.cpu(), views, (2.0, 2.0, 2.0), (0, 0, 0), out=out)
    cfg = _tiny_cfg()
    with pytest.raises(ValueError):
        RC.cgls(torch.ones(3, 9, 10, device=gpu), TINY_ANGLES, cfg, 2)     # one projection per angle
    with pytest.raises(ValueError):
        RC.ossart(torch.ones(6, 9, 10, device=gpu), TINY_ANGLES, cfg, 2, blocksize=0)
    with pytest.raises(ValueError):
        RC.tv_descent(out.double(), 0.1, 1)
    with pytest.raises(ValueError):
        RC.tv_descent(out, 0.1, -1)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())   # nothing was launched into it
