"""GPU: the geometry backward's row streaming at every edge it has.

raster_geom_backward_kernel gives one lane to a Gaussian; a wave concatenates the moment-row runs of its 64 Gaussians and streams
them through LDS GB_ROWS rows per pass (csrc/raster_geom.hip: 256 before, 320 since the rows are parked as 24 bytes), each lane
then adding ITS rows in row order.  The sums and their order do not depend on how the rows are parked or how long a pass is, the
translation unit is built without FMA contraction, so every gradient is a fixed function of the inputs, bit for bit.  Small
planted scenes put the streaming at its edges:

* sizes 1, 63, 64, 65, 255, 257: a partial last wave, a partial last workgroup, lanes past the end;
* tiny Gaussians (one tile each: 64 rows per wave, well inside one pass), wide ones (all 64 tiles of a 128^2 detector each: 4096
  rows per wave, 16 passes of 256 or 13 of 320, every Gaussian's run spans pass boundaries), a wave of exactly 256 rows and one
  of 258, a wave of exactly 320 rows and one of 322;
* culled Gaussians (zero rows) at the start of a wave, at its end, and as a whole wave, between visible ones;
* two stacked views (the batched instantiation shares the code).

The intended row counts are asserted from the CPU oracle's tiles_touched, so a scene cannot quietly stop meeting its edge.  Per
case: every returned gradient against the float64 oracle (oracle/parity.py, the bound of the other rasterizer tests), bit for bit
against tests/golden/geom_backward_passes.npz (recorded with tests/golden/make_geom_backward_passes.py on the commit BEFORE the
24-byte LDS rows, the 320-row passes and the five-workgroups-per-CU bound), and bit for bit against a second identical call.  The
two-view call equals its single-view calls bit for bit.
"""
import os

import numpy as np
import pytest
import torch

from r2_gaussian_amd import scene as S
from tests import helpers as Hh
from tests.test_raster_edges_gpu import _planted

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "geom_backward_passes.npz")
GRAD_NAMES = ("dL_dmeans2D", "dL_dopacity", "dL_dmu", "dL_dmeans3D", "dL_dcov3D", "dL_dscales", "dL_drotations")
TILE = 16
ANGLE = 0.6


# ------------------------------------------------------------------------------------------------ planted Gaussians
# a spec is _planted's (u, v, sigma_x, sigma_y, theta, view depth, density); the radius is ceil(3 sigma_max) pixels and the
# rectangle [(m - r) / 16, (m + r + 15) / 16) per axis, clipped to the grid (getRect, RAS/auxiliary.h)
def _tiny(g, W, H):
    """sigma 0.5 px about a tile centre: radius 2, one tile."""
    tx, ty = int(g.integers(0, W // TILE)), int(g.integers(0, H // TILE))
    return (TILE * tx + 8 + g.uniform(-3, 3), TILE * ty + 8 + g.uniform(-3, 3), 0.5, 0.5 * g.uniform(0.6, 1.0), g.uniform(0, np.pi),
            4.2 + 1.6 * g.random(), 0.05 + 0.2 * g.random())


def _wide(g, W, H):
    """sigma W / 3 about the detector's centre: the radius reaches past every border, all tiles."""
    return (W / 2 + g.uniform(-4, 4), H / 2 + g.uniform(-4, 4), W / 3.0, W / 3.0 * g.uniform(0.5, 1.0), g.uniform(0, np.pi),
            4.2 + 1.6 * g.random(), 0.02 + 0.05 * g.random())


def _corner(g, W, H, k, shift=0.0):
    """sigma 2.5 px (radius 8) on the k-th interior tile corner: 2 x 2 tiles; sigma 3.5 px (radius 11) 8 px further along x:
    3 x 2."""
    nx, ny = W // TILE - 1, H // TILE - 1
    cx, cy = 1 + k % nx, 1 + (k // nx) % ny
    s = 3.5 if shift else 2.5
    return (TILE * cx + shift, float(TILE * cy), s, s * g.uniform(0.6, 1.0), g.uniform(0, np.pi), 4.2 + 1.6 * g.random(),
            0.05 + 0.2 * g.random())


def _culled(g, W, H):
    """Behind the source: culled by the frustum test, no rows."""
    return (g.uniform(0, W), g.uniform(0, H), 2.0, 2.0, 0.0, -3.0 - g.random(), 0.1)


def _cloud(v, specs):
    xyz, sc, rot, den = _planted(v, specs)
    return S.Cloud(torch.from_numpy(xyz).contiguous(), torch.from_numpy(sc).contiguous(), torch.from_numpy(rot).contiguous(),
                   torch.from_numpy(den).contiguous())


def _case_tiny(P):
    def make():
        hw = (64, 64)
        v = S.make_view(ANGLE, hw)
        g = np.random.default_rng(1000 + P)
        want = dict(tiles=[1] * P)
        return _cloud(v, [_tiny(g, 64, 64) for _ in range(P)]), [v], want
    return make


def _case_wide(P):
    def make():
        hw = (128, 128)
        v = S.make_view(ANGLE, hw)
        g = np.random.default_rng(2000 + P)
        want = dict(tiles=[64] * P)
        return _cloud(v, [_wide(g, 128, 128) for _ in range(P)]), [v], want
    return make


def _case_rows(extra):
    """One wave of 64 Gaussians on tile corners, `extra` of them a tile column wider: 256 + 2 * extra rows."""
    def make():
        hw = (128, 128)
        v = S.make_view(ANGLE, hw)
        g = np.random.default_rng(3000 + extra)
        specs = [_corner(g, 128, 128, k) for k in range(64)]
        tiles = [4] * 64
        # (a corner in the grid's last column has no room for a third tile column: k % 7 == 6)
        for k in ([37] + [k for k in range(64) if k % 7 != 6 and k != 37])[:extra]:
            specs[k] = _corner(g, 128, 128, k, shift=8.0)
            tiles[k] = 6
        return _cloud(v, specs), [v], dict(tiles=tiles, wave_rows={0: 256 + 2 * extra})
    return make


def _mixed_specs(g, W, H, P, culled):
    """P Gaussians, the listed indices culled, the others tiny / corner / (every 11th) wide."""
    specs = []
    for i in range(P):
        if i in culled:
            specs.append(_culled(g, W, H))
        elif i % 11 == 5:
            specs.append(_wide(g, W, H))
        elif i % 3 == 0:
            specs.append(_corner(g, W, H, i))
        else:
            specs.append(_tiny(g, W, H))
    return specs


def _case_culled():
    def make():
        hw = (128, 128)
        v = S.make_view(ANGLE, hw)
        g = np.random.default_rng(4000)
        # wave 0: its first 9 lanes; wave 1: all of it; wave 2: its last 9 lanes, and a few single ones; wave 3 and the one
        # Gaussian of the second workgroup: visible
        culled = set(range(0, 9)) | set(range(64, 128)) | set(range(183, 192)) | {20, 21, 140, 150, 200}
        return _cloud(v, _mixed_specs(g, 128, 128, 257, culled)), [v], dict(culled=sorted(culled), min_wave_rows={0: 321, 2: 321, 3: 321},
                                                                          wave_rows={1: 0})
    return make


def _case_two_views():
    def make():
        hw = (128, 128)
        views = [S.make_view(ANGLE, hw), S.make_view(ANGLE + 0.15, hw)]
        g = np.random.default_rng(5000)
        culled = {0, 1, 30, 63, 64}
        return _cloud(views[0], _mixed_specs(g, 128, 128, 65, culled)), views, dict(culled=sorted(culled), min_wave_rows={0: 321})
    return make


CASES = {}
for _P in (1, 63, 64, 65, 255, 257):
    CASES["tiny_P%d" % _P] = _case_tiny(_P)
for _P in (1, 64, 65, 257):
    CASES["wide_P%d" % _P] = _case_wide(_P)
for _extra in (0, 1, 32, 33):   # 256 and 258 rows: the pass length the kernel had; 320 and 322: the one it has (GB_ROWS)
    CASES["rows_%d" % (256 + 2 * _extra)] = _case_rows(_extra)
CASES["culled_P257"] = _case_culled()
CASES["two_views_P65"] = _case_two_views()


def check_rows(o, want, view=0):
    """The oracle's tiles_touched are what the case was built for (view 0; a second view only has to stay multi-pass)."""
    tt = o["tiles_touched"].astype(np.int64)
    waves = [int(tt[i:i + 64].sum()) for i in range(0, tt.size, 64)]
    if view == 0:
        if "tiles" in want:
            assert tt.tolist() == want["tiles"], "tiles_touched is not the planted pattern: %s" % tt.tolist()
        for w, n in want.get("wave_rows", {}).items():
            assert waves[w] == n, "wave %d streams %d rows, meant %d" % (w, waves[w], n)
        for i in want.get("culled", ()):
            assert tt[i] == 0 and o["radii"][i] == 0, "Gaussian %d is not culled" % i
        if "culled" in want:
            vis = np.setdiff1d(np.arange(tt.size), want["culled"])
            assert (tt[vis] > 0).all(), "a Gaussian meant to be visible is culled"
    for w, n in want.get("min_wave_rows", {}).items():
        assert waves[w] >= n, "wave %d of view %d streams %d rows, meant more than one pass" % (w, view, waves[w])
    return waves


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _dL(V, hw):
    g = torch.Generator().manual_seed(3)
    return ((torch.rand((V,) + hw, generator=g) * 2 - 1) / float(hw[0] * hw[1])).numpy()


def run_single(c, v, dL, dev):
    """-> (forward state, gradients of two identical backward calls on it)."""
    h = Hh.hip_raster(c, v, dev)
    return h, Hh.hip_raster_backward(h, c, v, dL, dev), Hh.hip_raster_backward(h, c, v, dL, dev)


def run_batch(c, views, dL, dev):
    from r2_gaussian_amd import _C
    e = torch.empty(0)
    v0 = views[0]
    vm = torch.stack([v.world_view_transform for v in views]).to(dev)
    pm = torch.stack([v.full_proj_transform for v in views]).to(dev)
    a = (c.xyz.to(dev), c.density.to(dev), c.scales.to(dev), c.rotations.to(dev), 1.0, e, vm, pm, v0.tanfovx, v0.tanfovy,
         v0.image_height, v0.image_width, v0.mode, False)
    R, _color, radii, gb, bb, ib = _C.rasterize_gaussians_batch(*a)
    out = []
    for _ in range(2):
        res = _C.rasterize_gaussians_backward_batch(a[0], radii, a[2], a[3], 1.0, a[5], a[6], a[7], a[8], a[9],
                                                    torch.as_tensor(dL).to(dev), gb, R, bb, ib, a[12], False)
        torch.cuda.synchronize()
        out.append({n: t.cpu().numpy() for n, t in zip(GRAD_NAMES, res)})
    return R, out[0], out[1]


def record_case(name, dev):
    """What tests/golden/make_geom_backward_passes.py stores for a case: {"<case>/<view or batch>/<gradient>": array}."""
    c, views, _want = CASES[name]()
    hw = (views[0].image_height, views[0].image_width)
    dL = _dL(len(views), hw)
    rec = {}
    for k, v in enumerate(views):
        _h, g1, _g2 = run_single(c, v, dL[k:k + 1], dev)
        rec.update({"%s/view%d/%s" % (name, k, n): g1[n] for n in GRAD_NAMES})
    if len(views) > 1:
        _R, b1, _b2 = run_batch(c, views, dL, dev)
        rec.update({"%s/batch/%s" % (name, n): b1[n] for n in GRAD_NAMES})
    return rec


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def _assert_bits(got, golden, prefix, what):
    differ = []
    for n in GRAD_NAMES:
        ref = golden[prefix + n]
        assert got[n].shape == ref.shape, (n, got[n].shape, ref.shape)
        d = _bits(got[n]) != _bits(ref)
        if d.any():
            differ.append("%s (%d of %d words)" % (n, int(d.sum()), d.size))
    assert not differ, "%s: gradients differ from %s in: %s" % (prefix, what, differ)


# ------------------------------------------------------------------------------------------------ the tests
@pytest.mark.parametrize("name", [n for n in CASES if n != "two_views_P65"])
def test_single_view(name, oracle, gpu, golden):
    c, (v,), want = CASES[name]()
    hw = (v.image_height, v.image_width)
    o = Hh.oracle_raster(oracle, c, v)
    check_rows(o, want)
    dL = _dL(1, hw)
    h, g1, g2 = run_single(c, v, dL, gpu)
    assert np.array_equal(h["tiles_touched"], o["tiles_touched"])
    assert not [n for n in GRAD_NAMES if not np.array_equal(_bits(g1[n]), _bits(g2[n]))], "two identical calls differ"
    Hh.parity_raster_grads(oracle, o, g1, c, v, dL, "geom passes " + name)
    _assert_bits(g1, golden, name + "/view0/", "the recorded ones")


def test_two_stacked_views(oracle, gpu, golden):
    name = "two_views_P65"
    c, views, want = CASES[name]()
    hw = (views[0].image_height, views[0].image_width)
    P = c.xyz.shape[0]
    dL = _dL(len(views), hw)
    R, b1, b2 = run_batch(c, views, dL, gpu)
    assert not [n for n in GRAD_NAMES if not np.array_equal(_bits(b1[n]), _bits(b2[n]))], "two identical batched calls differ"
    _assert_bits(b1, golden, name + "/batch/", "the recorded ones")
    singles, rendered = [], 0
    for k, v in enumerate(views):
        o = Hh.oracle_raster(oracle, c, v)
        check_rows(o, want, view=k)
        h, g1, g2 = run_single(c, v, dL[k:k + 1], gpu)
        rendered += h["num_rendered"]
        assert not [n for n in GRAD_NAMES if not np.array_equal(_bits(g1[n]), _bits(g2[n]))], "two identical calls differ"
        Hh.parity_raster_grads(oracle, o, g1, c, v, dL[k:k + 1], "geom passes %s view %d" % (name, k))
        _assert_bits(g1, golden, "%s/view%d/" % (name, k), "the recorded ones")
        # the per-view rows of the stacked call are the single-view call's, bit for bit
        assert np.array_equal(_bits(b1["dL_dmeans2D"][k]), _bits(g1["dL_dmeans2D"])), "dL_dmeans2D of view %d" % k
        assert np.array_equal(_bits(b1["dL_dmu"][k]), _bits(g1["dL_dmu"].reshape(P))), "dL_dmu of view %d" % k
        singles.append(g1)
    assert R == rendered
    # summed over the views in view order, in float32 like the kernel's accumulators: the same adds, so the same bits
    for n in ("dL_dopacity", "dL_dmeans3D", "dL_dcov3D"):
        tot = np.zeros_like(singles[0][n])
        for gs in singles:
            tot = tot + gs[n]
        assert np.array_equal(_bits(b1[n]), _bits(tot.astype(np.float32))), "%s is not the sum of the single views" % n
    # the scale / rotation gradients come from ONE covariance backward on the summed dL/dcov3D (it is linear; the single views
    # round theirs separately): the bound tests/test_batch_gpu.py uses for the same comparison
    for n in ("dL_dscales", "dL_drotations"):
        tot = sum(gs[n].astype(np.float64) for gs in singles)
        scale = max(float(np.abs(tot).max()), 1e-30)
        assert float(np.abs(b1[n] - tot).max()) <= 2e-6 * scale, n
