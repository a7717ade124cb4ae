"""The yardstick of tests/test_fdk_edges_gpu.py, checked where no GPU is needed (tests/fdk_ref.py): in units of
eps32 * (W + H + 8) * T a float32 restatement of the back-projection kernel stays under K / 4 of the float64 oracle, a
half-pixel slip of the detector coordinate and a clamped (instead of zeroed) detector border are beyond 10 K, and the scenes
do put voxels where they are meant to: inside the detector, across each of its borders, and off it altogether.

Measured (worst over the 30 cases): restatement 1.20 units (5x16x65, detector 20x33, cone beam: the nearest voxel is 1.3 units in
front of the source); half-pixel slip >= 4,140 units in every case; clamped border >= 349 units in every case with a voxel at a
border."""
import numpy as np
import pytest

from tests import fdk_ref as R

BORDERS = ("u<0", "u>=W", "v<0", "v>=H")


def _has_border_voxels(sc):
    return any(sc["stats"]["straddle"].values())


@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_restatement_passes_and_planted_mistakes_fail(case):
    sc = R.scene(case)
    H, W, T, ref = sc["H"], sc["W"], sc["T"], sc["ref"]
    args = (sc["q"], sc["fp"], R.DSO, sc["n"], sc["s"], sc["ctr"], sc["cone"])
    good = R.backproject_f32(*args)
    r_good = R.worst_ratio(good, ref, T, H, W)
    r_shift = R.worst_ratio(R.backproject_f32(*args, shift_fx=0.5), ref, T, H, W)
    clamped = R.backproject_f32(*args, clamp_border=True)
    r_clamp = R.worst_ratio(clamped, ref, T, H, W)
    print("%s: restatement %.3f, half-pixel %.0f, clamped border %.0f units" % (R.case_id(case), r_good, r_shift, r_clamp))
    assert r_good <= R.K / 4, r_good
    assert (good[T == 0] == 0).all() and (ref[T == 0] == 0).all()   # nothing within a pixel of the footprint: exactly nothing
    assert r_shift > 10 * R.K, r_shift
    if _has_border_voxels(sc):
        assert r_clamp > 10 * R.K, r_clamp
    else:
        assert np.array_equal(clamped, good)   # no tap off the detector in any view: the planted clamp has nothing to act on


@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_every_scene_keeps_its_distance_and_its_voxel_classes(case):
    sc = R.scene(case)
    st = sc["stats"]
    # at hw ~ 0 float32 and float64 legitimately disagree: not what these scenes are for (a parallel beam has hw = 1)
    assert st["min_hw"] >= 1.0 - 1e-6, st["min_hw"]
    assert st["inside"].any()
    if case[0] in R.PAST_THE_DETECTOR:
        assert _has_border_voxels(sc)


@pytest.mark.parametrize("vol", list(R.VOLUMES))
def test_every_volume_meets_its_edges(vol):
    """Over a volume's three detectors and two beams (its six cases): some voxel is off the detector in every view (T == 0),
    some voxel's four taps lie across each of the four borders, and in some case a fifth of the voxels has all four taps on
    the detector in every view.  The first two are for the three volumes that reach past the detector
    (fdk_ref.PAST_THE_DETECTOR).  The side-6 volume cannot have a fifth inside (the detector sees about +-1.4 of its +-3 at
    the axis, 8 % at best): it has to keep a workgroup's worth, 256 voxels."""
    scs = [R.scene(c) for c in R.CASES if c[0] == vol]
    assert len(scs) == 6
    n, s, _ = R.VOLUMES[vol]
    inside = max(int(sc["stats"]["inside"].sum()) for sc in scs)
    if vol in R.PAST_THE_DETECTOR:
        assert any((sc["T"] == 0).any() for sc in scs)
        for b in BORDERS:
            assert any(sc["stats"]["straddle"][b] for sc in scs), b
    if max(s) >= 6.0:
        assert inside >= 256, inside
    else:
        assert inside >= 0.2 * np.prod(n), inside


def test_tap_bound_is_the_neighbourhood_maximum():
    """T on a scene small enough to do by hand: one view, one voxel at the centre of a parallel beam, a 4 x 6 detector."""
    from r2_gaussian_amd import scene as S
    fp = S.make_view(0.0, (4, 6), S.PARALLEL_BEAM).full_proj_transform.numpy()[None]
    q = np.zeros((1, 4, 6), np.float32)
    q[0, 0, 1] = -3.0    # the footprint is (fx, fy) = (2.5, 1.5): x0 = 2, y0 = 1, neighbourhood [1, 4] x [0, 3]
    q[0, 3, 0] = 7.0     # column 0 is outside it
    T, st = R.tap_bound(q, fp, R.DSO, (1, 1, 1), (2, 2, 2), (0, 0, 0), cone=False, return_stats=True)
    assert T.shape == (1, 1, 1) and T[0, 0, 0] == 3.0 and st["inside"].all() and not any(st["straddle"].values())
    q[0, 3, 0] = 0.0
    q[0, 0, 1] = 0.0
    assert R.tap_bound(q, fp, R.DSO, (1, 1, 1), (2, 2, 2), (0, 0, 0), cone=False)[0, 0, 0] == 0.0
