"""The Siddon projector (csrc/projector_siddon.hip) and its exact transpose (csrc/backprojector_siddon.hip) on the MI355X:
per-pixel agreement with the float64 restatement (tests/siddon_ref.py) within its derived float32 bound, the chord-length
anchor that separates the model from the interpolated one, the transpose bit for bit, the dot test, reproducibility, the
iterative algorithms against their float64 restatement on the dense Siddon matrix, the generator end to end, and the
untouched defaults."""
import json
import os

import numpy as np
import pytest
import torch

from r2_gaussian_amd import datagen as D
from r2_gaussian_amd import projector as K
from r2_gaussian_amd import recon as RC
from r2_gaussian_amd import scene as S
from tests import helpers as Hh
from tests import recon_ref as RR
from tests import siddon_ref as SR
from tests.operator_cases import TINY_ANGLES, TRANSPOSE, _tiny_cfg, one_hot_matrices, tiny_system

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
SID = "siddon"

# Hand-made parallel rays on a 6 x 5 x 4 grid of unit voxels, to force what camera matrices only approach: directions with
# exact zeros (flat axes) and crossings of two or three axes at exactly the same t.  {a, p00, pu, pv}; H x W = 7 x 9.
ALIGNED_N, ALIGNED_DET = (6, 5, 4), (7, 9)
ALIGNED = np.array([
    [1.0, 0.0, 0.0, -3.0, -0.75, -0.75, 0.0, 0.75, 0.0, 0.0, 0.0, 0.75],     # along +x: y and z flat
    [0.0, -1.0, 0.0, -0.75, 7.0, -0.75, 0.75, 0.0, 0.0, 0.0, 0.0, 0.75],     # along -y: x and z flat
    [0.0, 0.0, 2.0, -0.75, -0.75, -9.0, 0.0, 0.75, 0.0, 0.75, 0.0, 0.0],     # along +z, |d| = 2
    [1.0, 1.0, 0.0, -4.0, -2.0, -0.75, 0.5, -0.5, 0.0, 0.0, 0.0, 0.75],      # in-plane diagonal: x and y tie, z flat
    [-1.0, 1.0, 0.0, 7.0, -3.0, -0.75, 0.5, 0.5, 0.0, 0.0, 0.0, 0.75],       # the other diagonal, x decreasing
    [1.0, 1.0, 1.0, -3.0, -3.0, -3.0, 0.5, -0.5, 0.0, 0.0, 0.5, -0.5],       # space diagonal: triple ties
    [1.0, -1.0, -1.0, -2.0, 6.0, 5.0, 0.5, 0.5, 0.0, 0.5, 0.0, 0.5],         # mixed signs, triple ties
], np.float32)


def _aligned_forward(vol, dev):
    H, W = ALIGNED_DET
    return K.project_rays(vol, ALIGNED, False, H, W, (1.0, 1.0, 1.0), projection_type=SID)


def _aligned_adjoint(p, dev):
    return K.backproject_rays(p, ALIGNED, False, ALIGNED_N, (1.0, 1.0, 1.0), projection_type=SID)


def _check(got, ref, label):
    """Every compared pixel within its bound; misses exactly 0 unless the bound allows more.  -> stats."""
    px = ref["pixels"]
    g = got[px[:, 0], px[:, 1], px[:, 2]].astype(np.float64)
    err = np.abs(g - ref["value"])
    ratio = err / np.maximum(ref["bound"], 1e-300)
    st = {"pixels": int(len(g)), "hits": int(ref["hit"].sum()), "worst_err_over_bound": float(np.where(err > 0, ratio, 0).max()),
          "median_rel_bound": float(np.median((ref["bound"] / np.maximum(np.abs(ref["value"]), 1e-30))[ref["hit"]])),
          "unbounded_pixels": int((~np.isfinite(ref["bound"])).sum()),
          "max_n_seg": int(ref["n_seg"].max(initial=0))}
    Hh._log("siddon", label, lambda: st)
    print(label, st)
    assert (err <= ref["bound"]).all(), (label, st, int((err > ref["bound"]).sum()))
    return st


@pytest.mark.parametrize("case", TRANSPOSE, ids=[c[0] for c in TRANSPOSE])
def test_forward_agrees_with_the_restatement(gpu, case):
    name, scanner, det, n, s, ctr, angles, _ = case
    rng = np.random.RandomState(sum(n))
    vol = (rng.rand(*n) - 0.25).astype(np.float32)
    views = [S.make_view(a, det, scanner) for a in angles]
    got = K.project_views(torch.from_numpy(vol).to(gpu), views, s, ctr, projection_type=SID).cpu().numpy()
    rays32 = K.ray_params(views, s, ctr, n)
    ref = SR.project(vol, rays32, views[0].mode == 1, np.asarray(s, np.float64) / np.asarray(n), *det)
    st = _check(got, ref, "forward " + name)
    assert st["hits"] > 0
    if "misses" in name:
        assert st["hits"] < 0.8 * st["pixels"]


def test_forward_on_axis_aligned_rays_and_exact_ties(gpu):
    rng = np.random.RandomState(2)
    vol = (rng.rand(*ALIGNED_N) - 0.25).astype(np.float32)
    got = _aligned_forward(torch.from_numpy(vol).to(gpu), gpu).cpu().numpy()
    ref = SR.project(vol, ALIGNED, False, (1.0, 1.0, 1.0), *ALIGNED_DET)
    st = _check(got, ref, "forward axis-aligned")
    assert 0 < st["hits"] < st["pixels"]
    # a volume of ones: the chords of the axis-parallel views are the grid's extents times |d|, exactly
    ones = _aligned_forward(torch.ones(ALIGNED_N, device=gpu), gpu).cpu().numpy()
    for view, length in ((0, 6.0), (1, 5.0), (2, 4.0 * 2.0 / 2.0)):
        hit = ref["hit"].reshape(ones.shape)[view]
        assert hit.any() and (ones[view][hit] == np.float32(length)).all() and (ones[view][~hit] == 0).all()


@pytest.mark.parametrize("scanner", [S.CONE_BEAM, S.PARALLEL_BEAM], ids=["cone", "parallel"])
def test_full_size_sampled_pixels(gpu, scanner):
    """256^3 -> 512^2: every pixel computed, a seeded subset of 600 checked."""
    rng = np.random.RandomState(11)
    vol = rng.rand(256, 256, 256).astype(np.float32)
    views = [S.make_view(a, (512, 512), scanner) for a in (0.4, 2.2)]
    px = np.stack([rng.randint(0, 2, 600), rng.randint(0, 512, 600), rng.randint(0, 512, 600)], 1)
    px[:40, 1:] = 256   # the central rays, the longest chords
    s, ctr = (2.0, 2.0, 2.0), (0.0, 0.0, 0.0)
    got = K.project_views(torch.from_numpy(vol).to(gpu), views, s, ctr, projection_type=SID).cpu().numpy()
    rays32 = K.ray_params(views, s, ctr, vol.shape)
    ref = SR.project(vol, rays32, views[0].mode == 1, np.asarray(s) / 256.0, 512, 512, pixels=px)
    st = _check(got, ref, "256^3 -> 512^2 %s" % scanner["mode"])
    assert st["hits"] > 300 and st["max_n_seg"] > 256


@pytest.mark.parametrize("case", TRANSPOSE[:2] + TRANSPOSE[4:], ids=[c[0] for c in TRANSPOSE[:2] + TRANSPOSE[4:]])
def test_constant_volume_is_the_chord_and_separates_the_models(gpu, case):
    """A volume of ones gives the chord length within the bound (whose voxel-difference terms all vanish); the interpolated
    projector at accuracy 0.5 does not."""
    name, scanner, det, n, s, ctr, angles, _ = case
    views = [S.make_view(a, det, scanner) for a in angles]
    ones = torch.ones(n, device=gpu)
    rays32 = K.ray_params(views, s, ctr, n)
    ref = SR.project(np.ones(n), rays32, views[0].mode == 1, np.asarray(s, np.float64) / np.asarray(n), *det)
    assert np.abs(ref["value"] - ref["chord"]).max() <= 1e-12 * ref["chord"].max()
    sid = K.project_views(ones, views, s, ctr, projection_type=SID).cpu().numpy()
    st = _check(sid, ref, "chord anchor " + name)
    itp = K.project_views(ones, views, s, ctr, 0.5).cpu().numpy().reshape(-1).astype(np.float64)
    err = np.abs(itp - ref["chord"])
    over = err > ref["bound"]
    info = {"interpolated_over_bound": int(over.sum()), "interpolated_max_err": float(err.max()),
            "siddon_max_bound": float(ref["bound"].max())}
    Hh._log("siddon", "chord anchor interpolated " + name, lambda: info)
    hit = ref["hit"]
    assert st["hits"] > 0 and over.any() and np.median(err[hit]) > np.median(ref["bound"][hit]), info


def _same_bits(fwd, bwd, label):
    st = {"nonzero": int((fwd != 0).sum()), "pattern_differs": int(((fwd == 0) != (bwd == 0)).sum()),
          "entries_differ": int((fwd.view(np.uint32) != bwd.view(np.uint32)).sum()),
          "rays_missing": int((fwd == 0).all(1).sum()), "rays": int(fwd.shape[0])}
    Hh._log("siddon", label, lambda: st)
    print(label, st)
    assert st["pattern_differs"] == 0, (label, st)
    assert st["entries_differ"] == 0, (label, st)
    assert st["nonzero"] > 0
    return st


@pytest.mark.parametrize("case", TRANSPOSE, ids=[c[0] for c in TRANSPOSE])
def test_transpose_bit_for_bit(gpu, case):
    """A column by column from one-hot volumes through the forward, A^T row by row from one-hot pixels through the adjoint:
    the same zero pattern and the same bits (a sum with a single non-zero term rounds nowhere else), and A is the
    restatement's dense matrix within (8 u + the entry's endpoint errors)."""
    name, scanner, det, n, s, ctr, angles, _ = case
    views = [S.make_view(a, det, scanner) for a in angles]
    fwd, bwd = one_hot_matrices(gpu, views, det, n, s, ctr, projection_type=SID)
    st = _same_bits(fwd, bwd, "transpose " + name)
    if "misses" in name:
        assert st["rays_missing"] > 0.2 * st["rays"]
    # every row sums to the ray's chord: the entries are lengths, not merely equal on both sides
    rays32 = K.ray_params(views, s, ctr, n)
    ref = SR.project(np.ones(n), rays32, views[0].mode == 1, np.asarray(s, np.float64) / np.asarray(n), *det)
    assert (np.abs(fwd.astype(np.float64).sum(1) - ref["chord"]) <= ref["bound"] + 4 * U * ref["chord"]).all()


def test_transpose_bit_for_bit_on_axis_aligned_rays(gpu):
    H, W = ALIGNED_DET
    N, M = int(np.prod(ALIGNED_N)), len(ALIGNED) * H * W
    fwd, bwd = np.zeros((M, N), np.float32), np.zeros((M, N), np.float32)
    vol = torch.zeros(N, device=gpu)
    for v in range(N):
        vol.zero_()
        vol[v] = 1.0
        fwd[:, v] = _aligned_forward(vol.reshape(ALIGNED_N), gpu).reshape(-1).cpu().numpy()
    pr = torch.zeros(M, device=gpu)
    for r in range(M):
        pr.zero_()
        pr[r] = 1.0
        bwd[r] = _aligned_adjoint(pr.reshape(len(ALIGNED), H, W), gpu).reshape(-1).cpu().numpy()
    _same_bits(fwd, bwd, "transpose axis-aligned")
    # the entries of the axis-parallel views are |d| per crossed voxel, exactly; of the diagonal ones sqrt(2), sqrt(3)
    A = SR.dense_A_rays(ALIGNED, False, (1.0, 1.0, 1.0), ALIGNED_N, H, W)
    assert np.abs(fwd - A).max() <= 8 * U * A.max()


def test_dot_test_128(gpu):
    """<A x, y> = <x, A^T y> at 128^3 <-> 24 x 160^2 (cone, offset, anisotropic), within (n_max + P + V + 8) u sum |terms|:
    n_max = nx + ny + nz + 1 segments per ray, summed in order; P <= 64 pixels per voxel and view in the gather's box (a
    voxel's cube is at most 2.3 pixels wide on this detector: a box of at most 6 x 6); V views."""
    g = torch.Generator(device=gpu).manual_seed(0)
    n, det, V = (128, 128, 128), (160, 160), 24
    views = [S.make_view(a, det, S.CONE_BEAM) for a in np.linspace(0, 2 * np.pi, V + 1)[:-1] + 0.1]
    s, ctr = (2.0, 1.8, 2.1), (0.05, -0.02, 0.03)
    x = torch.rand(n, device=gpu, generator=g)
    y = torch.rand((V,) + det, device=gpu, generator=g)
    Ax = K.project_views(x, views, s, ctr, projection_type=SID)
    Aty = RC.backproject_views(y, views, s, ctr, nVoxel=n, projection_type=SID)
    lhs = float((Ax.double() * y.double()).sum())
    rhs = float((x.double() * Aty.double()).sum())
    terms = lhs   # x, y >= 0 and A >= 0: sum |terms| = <A x, y>
    n_max = sum(n) + 1
    bound = (n_max + 64 + V + 8) * U * terms
    st = {"rel_diff": abs(lhs - rhs) / terms, "bound_rel": bound / terms}
    Hh._log("siddon", "dot test 128^3 <-> 24 x 160^2", lambda: st)
    print("dot test", st)
    assert lhs > 0 and abs(lhs - rhs) <= bound, st


def test_bit_reproducible_and_independent_of_the_batch(gpu):
    rng = np.random.RandomState(4)
    n = (40, 33, 47)
    vol = torch.from_numpy(rng.rand(*n).astype(np.float32)).to(gpu)
    s, ctr = (2.0, 1.7, 2.2), (0.05, 0.0, -0.1)
    for scanner in (S.CONE_BEAM, S.PARALLEL_BEAM):
        views = [S.make_view(a, (70, 64), scanner) for a in np.linspace(0, 2 * np.pi, 7)[:-1]]
        a = K.project_views(vol, views, s, ctr, projection_type=SID)
        b = K.project_views(vol, views, s, ctr, projection_type=SID)
        one = torch.cat([K.project_views(vol, [v], s, ctr, projection_type=SID) for v in views])
        assert torch.equal(a, b) and torch.equal(a, one) and float(a.max()) > 0
        out = torch.full_like(a, float("nan"))
        assert K.project_views(vol, views, s, ctr, out=out, projection_type=SID) is out and torch.equal(out, a)
        # the adjoint: two calls, a NaN-filled out, and a view's contribution alone against the same view inside a batch
        p = torch.from_numpy(rng.rand(len(views), 70, 64).astype(np.float32)).to(gpu)
        v1 = RC.backproject_views(p, views, s, ctr, nVoxel=n, projection_type=SID)
        v2 = RC.backproject_views(p, views, s, ctr, out=torch.full(n, float("nan"), device=gpu), projection_type=SID)
        assert torch.equal(v1, v2) and float(v1.max()) > 0
        for k in (0, 3):
            alone = RC.backproject_views(p[k:k + 1], views[k:k + 1], s, ctr, nVoxel=n, projection_type=SID)
            masked = torch.zeros_like(p)
            masked[k] = p[k]
            assert torch.equal(RC.backproject_views(masked, views, s, ctr, nVoxel=n, projection_type=SID), alone)


def _tiny_system(mode):
    cfg = _tiny_cfg(mode)
    A = SR.dense_A_cfg(cfg, TINY_ANGLES)
    return cfg, A, tiny_system(cfg, A)


def _rel(a, b):
    return float(np.abs(np.asarray(a, np.float64) - b).max() / max(np.abs(b).max(), 1e-30))


@pytest.mark.parametrize("mode", ["cone", "parallel"])
def test_cgls_and_ossart_match_the_restatement_on_the_siddon_matrix(gpu, mode):
    """The tolerances of the interpolated tests (test_recon_gpu.py): 1e-4 of the largest value."""
    cfg, A, b = _tiny_system(mode)
    H, W = cfg["nDetector"]
    bt = torch.from_numpy(b.reshape(len(TINY_ANGLES), H, W)).to(gpu)
    # the operator is the dense matrix
    x = np.random.RandomState(1).rand(*cfg["nVoxel"]).astype(np.float32)
    op = RC.Operator(TINY_ANGLES, cfg, projection_type=SID)
    assert _rel(op.A(torch.from_numpy(x).to(gpu)).cpu().numpy().ravel(), A @ x.ravel().astype(np.float64)) < 1e-5
    assert _rel(op.At(bt).cpu().numpy().ravel(), A.T @ b.astype(np.float64)) < 1e-5
    xs, _ = RR.cgls(A, b.astype(np.float64), 4)
    st = {}
    for k in range(1, 5):
        st["cgls_%d" % k] = _rel(RC.cgls(bt, TINY_ANGLES, cfg, k, projection_type=SID).cpu().numpy().ravel(), xs[k - 1])
    for bs in (1, 4):
        want = RR.ossart(A, b.astype(np.float64), H * W, 2, bs, 1.0, 0.999)[-1]
        got = RC.ossart(bt, TINY_ANGLES, cfg, 2, bs, projection_type=SID).cpu().numpy().ravel()
        st["ossart_bs%d" % bs] = _rel(got, want)
    Hh._log("siddon", "algorithms vs float64 %s" % mode, lambda: st)
    print(mode, st)
    assert max(st.values()) < 1e-4, st
    # and through the dispatcher
    assert torch.equal(RC.reconstruct(bt, TINY_ANGLES, cfg, "cgls", projection_type=SID),
                       RC.cgls(bt, TINY_ANGLES, cfg, 60, projection_type=SID))


def test_generator_end_to_end(gpu, tmp_path):
    import yaml
    n = 16
    ax = -1 + (np.arange(n) + 0.5) * 2.0 / n
    X, Y, Z = np.meshgrid(ax, ax, ax, indexing="ij")
    vol = (0.8 * np.exp(-((X - 0.1) ** 2 + (Y + 0.2) ** 2 + Z ** 2) / 0.18)).astype(np.float32)
    cfg = dict(S.CONE_BEAM, nVoxel=[n, n, n], nDetector=[20, 24], accuracy=0.5, totalAngle=360.0, startAngle=0.0,
               noise=False, possion_noise=10000, gaussian_noise=[0, 10], sVoxel=[2.0, 2.0, 2.0], sDetector=[3.0, 3.6])
    np.save(str(tmp_path / "phantom.npy"), vol)
    with open(str(tmp_path / "scanner.yml"), "w") as f:
        yaml.safe_dump(cfg, f)
    case = D.main(["--vol", str(tmp_path / "phantom.npy"), "--scanner", str(tmp_path / "scanner.yml"), "--output",
                   str(tmp_path / "data"), "--n_train", "5", "--n_test", "3", "--seed", "2", "--projection_type", SID])
    meta = json.load(open(os.path.join(case, "meta_data.json")))
    assert meta["scanner"] == dict(cfg, projection_type=SID) and D.recorded_projection_type(meta["scanner"]) == SID
    rd = RC._read_case(case)
    for split in ("train", "test"):
        projs, angles = rd[split]
        want = K.project(vol, angles, cfg, projection_type=SID).cpu().numpy()
        assert projs.dtype == np.float32 and np.array_equal(projs, want)
        assert not np.array_equal(projs, K.project(vol, angles, cfg).cpu().numpy())
    # the recorded type alone selects the model; no type at all leaves the saved config as it was given
    again = D.generate(vol, meta["scanner"], str(tmp_path / "again"), "phantom", 5, 3, seed=2)
    assert np.array_equal(RC._read_case(again)["train"][0], rd["train"][0])
    plain = D.generate(vol, cfg, str(tmp_path / "plain"), "phantom", 5, 3, seed=2)
    assert json.load(open(os.path.join(plain, "meta_data.json")))["scanner"] == cfg
    assert np.array_equal(RC._read_case(plain)["train"][0], K.project(vol, rd["train"][1], cfg).cpu().numpy())


def test_defaults_are_untouched(gpu):
    """With the keyword absent, ``project`` and ``Operator`` give the bits of "interpolated"; "siddon" gives others and
    ignores ``accuracy``."""
    rng = np.random.RandomState(8)
    cfg = dict(S.CONE_BEAM, nVoxel=[24, 20, 22], nDetector=[30, 36], accuracy=0.5)
    vol = rng.rand(24, 20, 22).astype(np.float32)
    angles = np.linspace(0, 2 * np.pi, 6)[:-1] + 0.2
    a = K.project(vol, angles, cfg)
    assert torch.equal(a, K.project(vol, angles, cfg, projection_type="interpolated"))
    sid = K.project(vol, angles, cfg, projection_type=SID)
    assert not torch.equal(a, sid)
    assert torch.equal(sid, K.project(vol, angles, cfg, accuracy=0.1, projection_type=SID))
    assert torch.equal(sid, K.project(vol, angles, dict(cfg, accuracy=0.0), projection_type=SID))
    x = torch.from_numpy(vol).to(gpu)
    o0, o1, o2 = RC.Operator(angles, cfg), RC.Operator(angles, cfg, projection_type="interpolated"), \
        RC.Operator(angles, cfg, projection_type=SID)
    assert torch.equal(o0.A(x), o1.A(x)) and torch.equal(o0.A(x), a) and torch.equal(o2.A(x), sid)
    assert torch.equal(o0.At(a), o1.At(a)) and not torch.equal(o0.At(a), o2.At(a))
    assert torch.equal(RC.backproject(a, angles, cfg), o0.At(a))
    assert torch.equal(RC.backproject(a, angles, cfg, projection_type=SID), o2.At(a))
    assert torch.equal(RC.cgls(a, angles, cfg, 2), RC.cgls(a, angles, cfg, 2, projection_type="interpolated"))
