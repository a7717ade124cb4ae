"""The FDK kernels (csrc/fdk.hip) where a register-tiled kernel goes wrong: every padding, row-block and LDS size of the
filter's 8 x 8 tiling, bit for bit on integer data; its pre-weight and scale in ulps; the back-projection at partial
blocks and at the detector's borders in the unit of tests/fdk_ref.py; fdk() on an asymmetric, off-centre, rescaled scene."""
import numpy as np
import pytest
import torch

from oracle import fdk_oracle as F
from r2_gaussian_amd import _lib
from r2_gaussian_amd import fdk as K
from r2_gaussian_amd import scene as S
from r2_gaussian_amd._C import _stream
from tests import fdk_ref as R
from tests import helpers as Hh

pytestmark = pytest.mark.gpu

GUARD = 256          # sentinel floats on each side of the filter's output
SENTINEL = 12345.0


def _row_block(W):
    return 16 if W <= 1024 else (8 if W <= 2048 else 4)


def _filter_raw(gpu, x, taps, scale, cone=0, DSD=1.0, du=1.0, dv=1.0):
    """r2_fdk_filter on x [V,H,W] with the caller's taps, into a NaN-filled output that lies inside a larger buffer of
    sentinels.  -> out [V,W,H] (numpy); asserts that every element was written and none outside."""
    V, H, W = x.shape
    n = V * H * W
    buf = torch.full((GUARD + n + GUARD,), SENTINEL, dtype=torch.float32, device=gpu)
    out = buf[GUARD:GUARD + n]
    out.fill_(float("nan"))
    dx = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(gpu)
    dt = torch.from_numpy(np.ascontiguousarray(taps, dtype=np.float32)).to(gpu)
    L = _lib.lib()
    rc = L.r2_fdk_filter(V, H, W, dx.data_ptr(), dt.data_ptr(), float(scale), int(cone), float(DSD), float(du), float(dv),
                         out.data_ptr(), _stream(gpu))
    assert rc == 0, L.r2_last_error()
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    assert (host[:GUARD] == SENTINEL).all() and (host[GUARD + n:] == SENTINEL).all(), "written outside the output"
    got = host[GUARD:GUARD + n].reshape(V, W, H)
    assert not np.isnan(got).any(), "%d outputs never written" % int(np.isnan(got).sum())
    return got


def _int_filter_ref(x, taps):
    """out[v, i, r] = sum_j x[v, r, j] * taps[i - j + W - 1] in int64, transposed layout [V][W][H]."""
    V, H, W = x.shape
    xi, ti = x.astype(np.int64), taps.astype(np.int64)
    out = np.empty((V, W, H), np.int64)
    for v in range(V):
        for r in range(H):
            out[v, :, r] = np.convolve(xi[v, r], ti)[W - 1:2 * W - 1]
    return out


def _int_case(W, H, V=2):
    rng = np.random.RandomState(7 * W + H)
    x = rng.randint(-4, 5, size=(V, H, W)).astype(np.float32)
    taps = rng.randint(-8, 9, size=2 * W - 1).astype(np.float32)
    return x, taps


FILTER_WIDTHS = [1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 63, 65, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096]


@pytest.mark.parametrize("W", FILTER_WIDTHS)
def test_filter_indexing_is_exact_on_integers(gpu, W):
    """Inputs in [-4, 4], taps in [-8, 8]: every partial sum is an integer below 4096 * 32 = 2^17, so the float32 result is
    exact whatever the order of summation, fused or not -- any difference from the int64 convolution is an indexing mistake.
    Every W & 3 (the tap padding), W < 8 (a tile that is mostly padding), both sides of the row-block switches at 1024 and
    2048, the largest LDS request at 4096; H below, at and one past a row block; two views."""
    RB = _row_block(W)
    heights = (1, RB - 1, RB, RB + 1) if W < 1000 else (1, RB + 1)
    for H in heights:
        x, taps = _int_case(W, H)
        want = _int_filter_ref(x, taps)
        assert np.abs(want).max() < 2 ** 24
        got = _filter_raw(gpu, x, taps, 1.0)
        assert np.array_equal(got, want.astype(np.float32)), "W=%d H=%d: %d of %d outputs differ" % (
            W, H, int((got != want).sum()), want.size)
    again = _filter_raw(gpu, x, taps, 1.0)
    assert np.array_equal(got.view(np.uint32), again.view(np.uint32))


def test_filter_scale_is_applied_once(gpu):
    x, taps = _int_case(65, 17)
    want = _int_filter_ref(x, taps)
    got = _filter_raw(gpu, x, taps, 0.5)     # halves of integers below 2^17: still exact
    assert np.array_equal(got, (0.5 * want).astype(np.float32))


@pytest.mark.parametrize("W", [5, 130, 1025])
def test_filter_preweight_and_scale_in_ulps(gpu, W):
    """Hann taps (none of them zero), cone pre-weight, impulse rows: row r is 1.0 at column (37 r) % W and zero elsewhere
    (2.0 in the second view), so an output is the single product  preweight(r, j) * (taps[i - j + W - 1] * scale)  and the
    accumulation adds zeros.  du, dv and DSD are float32 values.

    Roundings of the kernel against the float64 value, in half-ulps u = 2^-24 of relative error: uu and vv one each, their
    squares and DSD^2 one more (3 u on a square), two additions of positive terms (+2 u: 5 u on the sum); the square root
    halves that and rounds (3.5 u), the division rounds (4.5 u), x *= (5.5 u), taps * scale (6.5 u), the product (7.5 u).  One
    ulp of a float32 is between 1 u and 2 u of its value, so 7.5 u is at most 7.5 ulp: the bound is 8 ulp.
    Measured on the MI355X: 2.14 ulp at most (W = 5: 1.12, 130: 1.97, 1025: 2.14)."""
    H = _row_block(W) + 1
    V, DSD, DSO, du, dv = 2, 7.0, 5.0, 0.015625 * 1.25, 0.03125 * 0.75
    x = np.zeros((V, H, W), np.float32)
    cols = (37 * np.arange(H)) % W
    x[0, np.arange(H), cols] = 1.0
    x[1, np.arange(H), cols] = 2.0
    taps = K.ramp_taps(W, H, "hann")
    assert (taps != 0).all()
    scale = np.float32(F.filter_scale(V, du, DSD, DSO))
    got = _filter_raw(gpu, x, taps, scale, cone=1, DSD=DSD, du=du, dv=dv)
    pw = F.preweight(H, W, dv, du, DSD)
    i = np.arange(W)[:, None]
    r = np.arange(H)[None, :]
    want = pw[r, cols[r]] * (taps.astype(np.float64)[i - cols[r] + W - 1] * float(scale))     # [W, H]
    want = np.stack([want, 2.0 * want])
    ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
    ulps = np.abs(got - want) / ulp
    Hh._log("fdk", "filter pre-weight W=%d H=%d" % (W, H), lambda: {"max_ulp": float(ulps.max())})
    print("W=%d: worst %.2f ulp" % (W, ulps.max()))
    assert ulps.max() <= 8.0, float(ulps.max())


def _backproject(gpu, sc):
    q_t = torch.from_numpy(np.ascontiguousarray(sc["q"].transpose(0, 2, 1))).to(gpu)
    fp = torch.from_numpy(sc["fp"].copy())
    return K.fdk_backproject(q_t, fp, R.DSO, sc["n"], sc["s"], sc["ctr"], sc["cone"]).cpu().numpy()


@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_backprojection_at_launch_edges_and_detector_borders(gpu, case):
    """|kernel - float64 oracle| <= K = 8 units of eps32 * (W + H + 8) * T (tests/fdk_ref.py; the unfused float32 restatement
    stays under 1.21, the planted mistakes are beyond 349), exactly zero where no view has a detector pixel within a pixel
    of the footprint, and the same bits twice.  Measured on the MI355X: 1.21 units at most (5x16x65, detector 64x96, cone)."""
    sc = R.scene(case)
    H, W, T, ref = sc["H"], sc["W"], sc["T"], sc["ref"]
    got = _backproject(gpu, sc)
    assert got.shape == tuple(sc["n"]) and np.isfinite(got).all()
    ratio = R.worst_ratio(got, ref, T, H, W)
    Hh._log("fdk", "backproject edges " + R.case_id(case), lambda: {"max_err_over_unit": ratio, "K": R.K})
    print("%s: %.3f units" % (R.case_id(case), ratio))
    assert ratio <= R.K, ratio
    assert (got[T == 0] == 0).all()
    assert np.array_equal(got.view(np.uint32), _backproject(gpu, sc).view(np.uint32))


# ------------------------------------------------------------------------------------------- fdk() away from symmetry
CFG = dict(S.CONE_BEAM, sDetector=[3.0, 4.0], nVoxel=[40, 32, 24], sVoxel=[2.0, 1.6, 1.2], offOrigin=[0.1, -0.05, 0.08],
           filter="hann")
N_VIEWS, DET_H, DET_W = 24, 36, 60


def _fdk_scene(mode):
    cfg = dict(CFG, mode=mode)
    cone = mode == "cone"
    rng = np.random.RandomState(11)
    projs = rng.rand(N_VIEWS, DET_H, DET_W).astype(np.float32)
    angles = np.linspace(0.0, 2.0 * np.pi, N_VIEWS + 1)[:-1]
    fp = np.stack([S.make_view(a, (DET_H, DET_W), cfg).full_proj_transform.numpy() for a in angles])
    # the reference's convention (dataset_readers.py:130): sDetector is [v, u]; its orthographic camera spans [-1, 1]
    du, dv = (4.0 / DET_W, 3.0 / DET_H) if cone else (2.0 / DET_W, 2.0 / DET_H)
    return cfg, cone, projs, angles, fp, du, dv


def _fdk_ref_and_bound(cfg, cone, projs, fp, du, dv):
    """The oracle's volume, and the bound: K units of the back-projection on the oracle's filtered rows plus the filter's
    1e-4 * sum |x| |taps| carried through the back-projection (its terms are all >= 0: the volume is their absolute sum)."""
    n, s, ctr, DSD, DSO = cfg["nVoxel"], cfg["sVoxel"], cfg["offOrigin"], cfg["DSD"], cfg["DSO"]
    qf = F.fdk_filter(projs, du, dv, DSD, DSO, cfg["filter"], cone)
    ref = F.fdk_backproject(qf, fp, DSO, n, s, ctr, cone)
    T = R.tap_bound(qf, fp, DSO, n, s, ctr, cone)
    t = np.abs(F.spatial_taps(DET_W, DET_H, cfg["filter"]))
    xw = np.abs(projs) * F.preweight(DET_H, DET_W, dv, du, DSD, cone)[None]
    e = np.stack([[np.convolve(xw[v, r], t)[DET_W - 1:2 * DET_W - 1] for r in range(DET_H)] for v in range(N_VIEWS)])
    e *= 1e-4 * F.filter_scale(N_VIEWS, du, DSD, DSO, cone)
    bound = R.K * R.unit(T, DET_H, DET_W) + F.fdk_backproject(e, fp, DSO, n, s, ctr, cone)
    return ref, bound


@pytest.mark.parametrize("mode", ["cone", "parallel"])
def test_fdk_on_an_asymmetric_off_centre_scene(gpu, mode):
    """Detector 36 x 60 of size [3, 4], volume 40 x 32 x 24 of size [2, 1.6, 1.2] off the origin, Hann filter: nothing here is
    square, cubic or centred, so du/dv, H/W, the voxel pitches and the offset cannot be exchanged unnoticed."""
    cfg, cone, projs, angles, fp, du, dv = _fdk_scene(mode)
    ref, bound = _fdk_ref_and_bound(cfg, cone, projs, fp, du, dv)
    got = K.fdk(projs, angles, cfg, device=gpu).cpu().numpy()
    assert got.shape == (40, 32, 24)
    err = np.abs(got - ref)
    ratio = float((err / (bound + 1e-300)).max())
    Hh._log("fdk", "fdk asymmetric " + mode, lambda: {"max_err_over_bound": ratio})
    assert (err <= bound).all(), ratio
    # the bound can tell du from dv
    swapped = F.fdk(projs, fp, dv, du, cfg["DSD"], cfg["DSO"], cfg["nVoxel"], cfg["sVoxel"], cfg["offOrigin"], cfg["filter"], cone)
    assert not (np.abs(got - swapped) <= bound).all()


def test_fdk_scene_scale(gpu):
    """Every length doubled: fdk() normalises the scene by 2 / max(sVoxel) = 0.5 and multiplies the projections by it, so the
    same projections reconstruct to half the original scene's volume -- within the original's bound, halved."""
    cfg, cone, projs, angles, fp, du, dv = _fdk_scene("cone")
    ref, bound = _fdk_ref_and_bound(cfg, cone, projs, fp, du, dv)
    big = dict(cfg, DSD=2 * cfg["DSD"], DSO=2 * cfg["DSO"], sDetector=[2 * s for s in cfg["sDetector"]],
               sVoxel=[2 * s for s in cfg["sVoxel"]], offOrigin=[2 * o for o in cfg["offOrigin"]])
    got = K.fdk(projs, angles, big, device=gpu).cpu().numpy()
    err = np.abs(got - 0.5 * ref)
    ratio = float((err / (0.5 * bound + 1e-300)).max())
    Hh._log("fdk", "fdk scene scale 0.5", lambda: {"max_err_over_bound": ratio})
    assert (err <= 0.5 * bound).all(), ratio


def test_launch_limits_are_refused(gpu):
    """Grid dimensions y and z hold 65535 blocks: more views, or a larger volume, is an error before any launch (the buffers
    are never touched, so one float serves for all of them)."""
    L = _lib.lib()
    one = torch.zeros(16, dtype=torch.float32, device=gpu)
    p, st = one.data_ptr(), _stream(gpu)
    assert L.r2_fdk_filter(65536, 1, 1, p, p, 1.0, 0, 1.0, 1.0, 1.0, p, st) == _lib.R2_ERR_INVALID
    assert b"65535 views" in L.r2_last_error()
    for nx, ny in ((65536, 1), (1, 16 * 65535 + 1)):
        rc = L.r2_fdk_backproject(1, 1, 1, p, p, 1, 5.0, nx, ny, 1, 2.0, 2.0, 2.0, 0.0, 0.0, 0.0, p, st)
        assert rc == _lib.R2_ERR_INVALID
        assert b"volume too large for one launch" in L.r2_last_error()
    torch.cuda.synchronize()
