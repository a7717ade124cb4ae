"""CPU: the float64 restatement of the voxel render (tests/voxel_ref.py) checked without a GPU -- against hand-computed values,
against the CPU oracle on every scene of tests/voxel_scenes.py, and against a volume with one pair removed (the bound must catch
it)."""
import math

import numpy as np
import pytest

from tests import helpers as Hh
from tests import voxel_ref as VR
from tests import voxel_scenes as VS


def _oracle_ref(oracle, sc, gi, dL=None):
    n, s, ctr = sc.grids[gi]
    o = Hh.oracle_voxel(oracle, sc.cloud, n, s, ctr)
    co = o["conic_opacity"]
    return o, VR.render(o["means3D_norm"], co[:, :6], co[:, 6], o["point_list"], o["ranges"], n, dL=dL,
                        sVoxel=s if dL is not None else None)


def test_one_gaussian_by_hand():
    """One Gaussian centred on voxel (4, 4, 4) of an 8^3 grid; its neighbour along x sits 1e-4 above the cut-off, the one along
    y 1e-4 below (D = 1 + 2 ln(1.0001 / 0.9999)); through the off-diagonal C the x-z diagonal neighbour (+1, +1) is 5 % above the
    cut-off, the other diagonal far below it."""
    f = np.float32
    op = f(1.0001e-6 * math.exp(0.5))
    A, B, C, D, E, F = f(1.0), f(0.0), f(-0.45), f(1.0 + 2.0 * math.log(1.0001 / 0.9999)), f(0.0), f(0.8)
    mean = np.array([[4.5, 4.5, 4.5]], np.float32)
    conic = np.array([[A, B, C, D, E, F]], np.float32)
    n = (8, 8, 8)
    ranges = np.array([[0, 1]], np.uint32)
    ref = VR.render(mean, conic, np.array([op]), np.array([0], np.uint32), ranges, n,
                    dL=np.ones(n, np.float32))
    vid = lambda x, y, z: (x * 8 + y) * 8 + z   # noqa: E731
    A64, C64, D64, F64, op64 = (float(v) for v in (A, C, D, F, op))
    hand = {vid(4, 4, 4): op64,
            vid(5, 4, 4): op64 * math.exp(-0.5 * A64),                               # 1.0001e-6: in
            vid(4, 5, 4): 0.0,                                                       # 0.9999e-6: out
            vid(5, 4, 5): op64 * math.exp(-0.5 * (A64 + F64) - C64),                 # 1.05e-6: in
            vid(3, 4, 5): 0.0}                                                       # 4e-7: out
    assert op64 * math.exp(-0.5 * A64) > 1.00009e-6 and op64 * math.exp(-0.5 * D64) < 0.99991e-6
    for v, want in hand.items():
        assert ref["value"][v] == pytest.approx(want, rel=1e-13, abs=0.0), v
        assert ref["n_band"][v] == 0
    live = [v for v, want in hand.items() if want > 0]
    assert (ref["n_pairs"][live] == 1).all() and ref["n_pairs"][vid(4, 5, 4)] == 0
    # one term: no summation error, the bound is the pair's own exponent error -- a few hundred u of alpha at most
    assert (ref["bound"][live] < 5e-5 * ref["value"][live]).all() and (ref["bound"][live] > 0).all()
    # nothing else is above the cut-off but the centre, +-x, +-z and the (+1, +1) / (-1, -1) x-z diagonals
    want_live = sum(1 for x in range(8) for y in range(8) for z in range(8)
                    if op64 * math.exp(-0.5 * (A64 * (x - 4) ** 2 + D64 * (y - 4) ** 2 + F64 * (z - 4) ** 2) - C64 * (x - 4) * (z - 4)) >= VR.ALPHA_MIN32)
    assert int((ref["value"] > 0).sum()) == want_live == 7
    # dL/dopacity with dL = 1: the sum of exp(power) over the live pairs
    assert ref["dop"][0] == pytest.approx(ref["value"].sum() / op64, rel=1e-12)


@pytest.mark.parametrize("name", list(VS.SCENES))
def test_oracle_within_the_bound_on_every_scene(name, oracle):
    sc = VS.SCENES[name]()
    for gi, (n, s, ctr) in enumerate(sc.grids):
        rng = np.random.default_rng(gi)
        dL = (rng.uniform(-1.0, 1.0, n) / np.prod(n)).astype(np.float32)
        o, ref = _oracle_ref(oracle, sc, gi, dL=dL)
        assert o["num_rendered"] > 0 and o["vol"].max() > 0
        what = "%s %s" % (name, "x".join(map(str, n)))
        VR.check(o["vol"], ref, what)
        tight, nonempty = VR.tightness(ref)
        assert nonempty > 1000 and tight >= 0.95, (what, tight, nonempty)
        sums = oracle.voxel_backward_audit(o, dL)[0]
        VR.check_dop(sums[:, 9], ref, what)   # the oracle's dL/dopacity terms, summed in double
        g = oracle.voxel_backward(o, sc.cloud.scales.numpy(), sc.cloud.rotations.numpy(), 1.0, None, dL, acc64=True)
        VR.check_dmean(g["dL_dmeans3D"], ref, what)


def test_a_missing_pair_breaks_the_check(oracle):
    """Negative control: take one live pair out of each of 100 seeded voxels of the oracle volume (the smallest one outside the
    band, among the voxels where the bound claims to see it), or count it twice: every one of them must fail the check."""
    sc = VS.lists_scene()
    o, ref = _oracle_ref(oracle, sc, 0)
    VR.check(o["vol"], ref, "lists")
    tight = np.nonzero(np.isfinite(ref["min_out"]) & (ref["bound"].astype(np.float64) < ref["min_out"]))[0]
    pick = np.random.default_rng(5).choice(tight, 100, replace=False)
    vol = o["vol"].reshape(-1)
    for v in pick:
        one = {k: (a[[v]] if isinstance(a, np.ndarray) and a.shape[:1] == vol.shape else a) for k, a in ref.items()}
        dropped = np.float32(np.float64(vol[v]) - ref["min_out"][v])
        with pytest.raises(AssertionError):
            VR.check([dropped], one, "voxel %d without its smallest pair" % v)
    # and duplicating that pair instead is caught just the same
    for v in pick:
        one = {k: (a[[v]] if isinstance(a, np.ndarray) and a.shape[:1] == vol.shape else a) for k, a in ref.items()}
        with pytest.raises(AssertionError):
            VR.check([np.float32(np.float64(vol[v]) + ref["min_out"][v])], one, "voxel %d with a pair twice" % v)
