"""GPU: the two optional inputs of the reference's ABI -- a precomputed covariance (cov3D_precomp in place of scales + rotations)
and a scale_modifier other than 1 -- on EVERY chain of both operators.  Each fast chain has its own copy of the geometry kernels
(rasterizer: general and tile-first preprocess, single-view and multi-view geometry backward; voxelizer: general, small-grid and
stick-first preprocess, x-slab calls), and csrc/dispatch.hpp promises that results never depend on the chain.

Settings: `mod07` and `mod16` pass scales + rotations at modifier 0.7 / 1.6; `precomp` passes a covariance built from ANOTHER
cloud's scales and rotations at 1.3 (so nothing can be recovered from the scales that are passed), with 1.3 as the modifier
argument, which the kernels must then ignore.

Every chain is named by its r2_path_stats counter.  The oracle (pinned to the reference on these inputs by
tests/test_oracle_vs_ref.py and the voxel_mod / voxel_precomp fixtures) gives the lists, the volume / image and the gradients;
the bounds are those of tests/test_voxel_gpu.py, tests/test_raster_gpu.py and tests/test_batch_gpu.py.  Before a parity is
trusted, the oracle's own output for the setting is shown to differ from the output WITHOUT the setting (modifier 1.0; for
`precomp` the covariance of the cloud's own scales and rotations at 1.0 and at 1.3) by more than 100 x the tolerance the parity
applies (oracle/parity.py) at more than half of the visible voxels / pixels / rows: a kernel that ignored the input cannot pass."""
import functools

import numpy as np
import pytest
import torch

from r2_gaussian_amd import scene as S
from tests import helpers as Hh

pytestmark = pytest.mark.gpu

P = 3000
N_FAR = 300                                            # rasterizer only: Gaussians near the source orbit, see _raster_cloud
SETTINGS = {"mod07": 0.7, "mod16": 1.6, "precomp": 1.3}   # name -> the modifier argument of the call
VOXEL_SCALE_MULT, RASTER_SCALE_MULT = 0.7, 1.5
# 18 tiles: the small-grid path, and the general chain through two x-slab calls
GRID_SMALL = ((20, 16, 24), (0.8, 0.6, 0.9), (0.3, -0.25, 0.2))
# 225 tiles: the stick-first chain, and the general chain with r2_voxel_sticks_control(0)
GRID_LARGE = ((72, 40, 33), (1.2, 0.7, 0.6), (0.3, -0.25, 0.2))
GRIDS = {"20x16x24": GRID_SMALL, "72x40x33": GRID_LARGE}
HW = (80, 96)
ANGLES = tuple(0.3 + 0.9 * k for k in range(3))
SCANNERS = {"cone": S.CONE_BEAM, "parallel": S.PARALLEL_BEAM}
# parallel beam at modifier 1.6 is left out: its flip candidates (0.92 % of the pixels) sit too close to the 1 % cap
RASTER_CASES = [("mod07", "cone"), ("mod16", "cone"), ("precomp", "cone"), ("mod07", "parallel"), ("precomp", "parallel")]
VOXEL_GRADS = ("dL_dopacity", "dL_dmeans3D", "dL_dcov3D", "dL_dscales", "dL_drotations")
RASTER_GRADS = ("dL_dmeans2D", "dL_dopacity", "dL_dmu", "dL_dmeans3D", "dL_dcov3D", "dL_dscales", "dL_drotations")
GEOM_ONLY = ("dL_dscales", "dL_drotations")            # absent from the parity's statistics under a precomputed covariance

sticks_mode = pytest.fixture(Hh.sticks_mode)


# ------------------------------------------------------------------------------------------------ inputs (CPU, built once)
@functools.lru_cache(maxsize=None)
def _voxel_cloud():
    """The small-grid path is built for patches that most of the cloud misses: its lists live in the radix sort's workspace, which
    is sized by P (csrc/voxel_small.hip, SmallTmp: 7406 instances at P = 3000), beyond that the call hands over to the general
    chain.  With at most half of the rows culled that leaves under five tiles per visible Gaussian on the 18-tile grid: hence
    the small scales (5766 instances there), and the positions pulled a little towards the grids' centre to keep the culled
    share below 50 %."""
    c = S.make_cloud(P, seed=31, scale_mult=VOXEL_SCALE_MULT)
    ctr = torch.tensor(GRID_SMALL[2])
    return c._replace(xyz=(ctr + 0.9 * (c.xyz - ctr)).contiguous())


@functools.lru_cache(maxsize=None)
def _raster_cloud():
    """S.make_cloud plus N_FAR Gaussians at radius 6..7 from the isocentre, around the source orbit (radius 5): each view has
    another arc of them behind its near plane, so every view culls a different, non-empty subset."""
    c = S.make_cloud(P, seed=32, scale_mult=RASTER_SCALE_MULT)
    far = S.make_cloud(N_FAR, seed=33, scale_mult=RASTER_SCALE_MULT * (N_FAR / P) ** (1.0 / 3.0))   # the main cloud's scales
    g = torch.Generator().manual_seed(34)
    phi = torch.rand(N_FAR, generator=g) * (2.0 * np.pi)
    rad = 6.0 + torch.rand(N_FAR, generator=g)
    z = torch.rand(N_FAR, generator=g) - 0.5
    xyz = torch.stack([rad * torch.cos(phi), rad * torch.sin(phi), z], 1).float()
    cat = lambda a, b: torch.cat([a, b], 0).contiguous()   # noqa: E731
    return S.Cloud(cat(c.xyz, xyz), cat(c.scales, far.scales), cat(c.rotations, far.rotations), cat(c.density, far.density))


@functools.lru_cache(maxsize=None)
def _precomp(op):
    """The covariance of the `precomp` setting: another cloud's scales and rotations at 1.3, one row per Gaussian of `op`'s cloud."""
    from oracle import oracle as O
    c = _voxel_cloud() if op == "voxel" else _raster_cloud()
    n = c.xyz.shape[0]
    other = S.make_cloud(n, seed=1031 if op == "voxel" else 1032,
                         scale_mult=VOXEL_SCALE_MULT if op == "voxel" else RASTER_SCALE_MULT)
    return O.cov3d(other.scales.numpy(), SETTINGS["precomp"], other.rotations.numpy())


def _inputs(op, setting):
    """-> the keyword arguments of the helpers for the setting."""
    return dict(scale_modifier=SETTINGS[setting], cov3D_precomp=_precomp(op) if setting == "precomp" else None)


def _baselines(op, setting):
    """What the call would compute if the setting were ignored: [(label, helper keyword arguments)]."""
    if setting != "precomp":
        return [("modifier 1.0", dict(scale_modifier=1.0))]
    return [("own scales at 1.0", dict(scale_modifier=1.0)), ("own scales at 1.3", dict(scale_modifier=SETTINGS["precomp"]))]


def _voxel_dL(n):
    g = torch.Generator().manual_seed(7)
    return ((torch.rand(*n, generator=g) * 2 - 1) / float(np.prod(n))).numpy()


def _view(beam, k):
    return S.make_view(ANGLES[k], HW, SCANNERS[beam])


def _means3D_ref_and_tol(chain, sums, width):
    """dL_dmeans3D of the oracle (its double sums through the geometry chain) and the tolerance oracle/parity.py applies to it:
    |J| (1e-4 sum|terms| + flip budget + 1e-6 |sum|), J the chain's Jacobian column by column."""
    s, a, f = sums
    ref = chain(s.astype(np.float32))["dL_dmeans3D"].astype(np.float64)
    tol = np.zeros_like(ref)
    for q in range(width):
        unit = np.zeros(s.shape, np.float32)
        unit[:, q] = 1.0
        tol += np.abs(chain(unit)["dL_dmeans3D"].astype(np.float64)) * (1e-4 * a[:, q:q + 1] + f[:, q:q + 1] + 1e-6 * np.abs(s[:, q:q + 1]))
    return ref, tol


def _sensitive(label, got, base, tol, visible):
    """More than half of the visible elements (rows: any component) differ from the baseline by more than 100 x the tolerance."""
    far = np.abs(np.asarray(got, np.float64) - np.asarray(base, np.float64)) > 100.0 * tol
    if far.ndim == 2 and visible.ndim == 1:
        far = far.any(axis=1)
    frac = float(far[visible].mean())
    assert visible.sum() > 100 and frac > 0.5, "%s: only %.3f of %d visible elements differ by > 100 x tolerance" % (
        label, frac, int(visible.sum()))
    return frac


@functools.lru_cache(maxsize=None)
def _voxel_oracle(setting, grid):
    """-> (oracle state, dL, statistics of the conditions).  Checked with the oracle alone: 1..50 % of the rows are culled, and the
    setting changes the volume and dL_dmeans3D by far more than the tolerances."""
    from oracle import oracle as O
    c = _voxel_cloud()
    n, s, ctr = GRIDS[grid]
    kw = _inputs("voxel", setting)
    o = Hh.oracle_voxel(O, c, n, s, ctr, **kw)
    culled = (o["radii_x"] == 0) & (o["radii_y"] == 0) & (o["radii_z"] == 0)
    assert np.array_equal(culled, o["tiles_touched"] == 0)
    frac_culled = float(culled.mean())
    assert 0.01 <= frac_culled <= 0.5, (setting, grid, frac_culled)
    dL = _voxel_dL(n)
    sc, q = (c.scales.numpy(), c.rotations.numpy()) if kw["cov3D_precomp"] is None else (None, None)
    chain = lambda raw: O.voxel_geom_chain(o, raw, sc, q, kw["scale_modifier"], kw["cov3D_precomp"])   # noqa: E731
    ref, tol = _means3D_ref_and_tol(chain, O.voxel_backward_audit(o, dL), 9)
    budget, _nb = O.voxel_forward_audit(o)
    stats = dict(culled=frac_culled, peak=float(o["vol"].max()))
    for label, bkw in _baselines("voxel", setting):
        b = Hh.oracle_voxel(O, c, n, s, ctr, **bkw)
        for k in ("radii_x", "radii_y", "radii_z"):   # quirk Q5: the radii come from the raw scales -- no modifier, no covariance
            assert np.array_equal(o[k], b[k]), (setting, grid, k)
        what = "voxel %s %s vs %s" % (setting, grid, label)
        stats["vol differs, " + label] = _sensitive(what + " (volume)", o["vol"], b["vol"], 1e-4 * np.abs(o["vol"]) + budget,
                                                    o["vol"] > 0)
        bchain = lambda raw: O.voxel_geom_chain(b, raw, c.scales.numpy(), c.rotations.numpy(), bkw["scale_modifier"], None)   # noqa: E731
        bref, _ = _means3D_ref_and_tol(bchain, O.voxel_backward_audit(b, dL), 0)
        stats["dL_dmeans3D differs, " + label] = _sensitive(what + " (dL_dmeans3D)", ref, bref, tol, ~culled)
        stats["peak, " + label] = float(b["vol"].max())
    return o, dL, stats


@functools.lru_cache(maxsize=None)
def _raster_oracle(setting, beam, k):
    from oracle import oracle as O
    c = _raster_cloud()
    v = _view(beam, k)
    kw = _inputs("raster", setting)
    o = Hh.oracle_raster(O, c, v, **kw)
    culled = o["radii"] == 0
    frac_culled = float(culled.mean())
    assert 0.01 <= frac_culled <= 0.5, (setting, beam, k, frac_culled)
    dL = S.make_pixel_grad(*HW, seed=11 + k).numpy()
    xyz, _rho, sc, q = Hh.cloud_np(c)
    vm, pm = Hh.np_view(v)

    def chain_of(st, sc, q, mod, cov):
        return lambda raw: O.raster_geom_chain(st, raw, xyz, sc, q, mod, cov, vm, pm, v.tanfovx, v.tanfovy)
    own = (None, None) if kw["cov3D_precomp"] is not None else (sc, q)
    ref, tol = _means3D_ref_and_tol(chain_of(o, own[0], own[1], kw["scale_modifier"], kw["cov3D_precomp"]),
                                    O.raster_backward_audit(o, dL), 7)
    budget, _nb = O.raster_forward_audit(o)
    stats = dict(culled=frac_culled, peak=float(o["color"].max()))
    for label, bkw in _baselines("raster", setting):
        b = Hh.oracle_raster(O, c, v, **bkw)
        what = "raster %s %s view %d vs %s" % (setting, beam, k, label)
        stats["image differs, " + label] = _sensitive(what + " (image)", o["color"], b["color"],
                                                      1e-4 * np.abs(o["color"]) + budget, o["color"] > 0)
        bref, _ = _means3D_ref_and_tol(chain_of(b, sc, q, bkw["scale_modifier"], None), O.raster_backward_audit(b, dL), 0)
        stats["dL_dmeans3D differs, " + label] = _sensitive(what + " (dL_dmeans3D)", ref, bref, tol, ~culled)
        stats["peak, " + label] = float(b["color"].max())
    return o, dL, stats


def test_culled_subsets_differ_between_views():
    """Every view culls another subset of the rasterizer's cloud (the Gaussians around the source orbit)."""
    for beam in SCANNERS:
        sets = [frozenset(np.nonzero(_raster_oracle("mod07", beam, k)[0]["radii"] == 0)[0]) for k in range(len(ANGLES))]
        assert len(set(sets)) == len(sets) and all(sets), beam


# ------------------------------------------------------------------------------------------------ shared checks
def _bitwise(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _poison(dev, floats):
    """Allocate, NaN-fill and free blocks of the size the backward is about to allocate for its gradients (torch.empty, the kernels
    must write every row): the recycled memory is then not zero by luck."""
    blocks = [torch.full((floats,), float("nan"), device=dev) for _ in range(3)]
    torch.cuda.synchronize()
    del blocks


def _assert_caps(label, st, n_elements=None):
    """The conditions the inputs must keep for the checks to mean what they say."""
    if n_elements is None:
        af = st["after_flips"]
        assert not af["pair_list_truncated"], label
        assert af["rows_skipped_many_pairs"] == 0, (label, af)   # no flagged row holds more than 8 borderline pairs
    else:
        assert st["n_flip_candidates"] < 0.01 * n_elements, (label, st)


def _grad_margins(keys, sg, label, precomp):
    worst = 0.0
    for k in keys:
        if precomp and k in GEOM_ONLY:
            assert k not in sg
            continue
        assert sg[k]["max_err_over_scale_unflagged"] <= 2e-4, (label, k, sg[k])
        worst = max(worst, sg[k]["max_err_over_tol_unflagged"])
    return dict(worst_err_over_tol_unflagged=worst, after_flips=sg["after_flips"]["max_err_over_tol_after_flips"],
                worst_err_over_scale_unflagged=max(sg[k]["max_err_over_scale_unflagged"] for k in keys if k in sg),
                rows_flagged=sg["after_flips"]["rows_flagged"])


def _assert_zero_rows(gh, n_rows, label):
    for k in GEOM_ONLY:
        a = np.asarray(gh[k]).reshape(n_rows, -1)
        assert np.array_equal(a.view(np.uint32) & np.uint32(0x7FFFFFFF), np.zeros(a.shape, np.uint32)), \
            "%s: %s is not zero in %d rows under a precomputed covariance" % (label, k, int((a != 0).any(1).sum() + np.isnan(a).any(1).sum()))


# ------------------------------------------------------------------------------------------------ voxelizer
@pytest.mark.parametrize("grid", list(GRIDS))
@pytest.mark.parametrize("setting", list(SETTINGS))
def test_voxelizer_every_chain(setting, grid, oracle, gpu, sticks_mode):
    c = _voxel_cloud()
    n, s, ctr = GRIDS[grid]
    kw = _inputs("voxel", setting)
    precomp = kw["cov3D_precomp"] is not None
    o, dL, cond = _voxel_oracle(setting, grid)
    Hh._log("optional_inputs", "voxel %s %s conditions" % (setting, grid), lambda: cond)
    nvox = int(np.prod(n))
    # the debug call (general chain): radii, lists, and the covariance the state holds
    d, sv = Hh.served(lambda: Hh.hip_voxel(c, n, s, ctr, gpu, debug=True, **kw))
    assert sv == {"voxel.general.debug": 1}, sv
    assert d["num_rendered"] == o["num_rendered"] > 0
    for k in ("radii_x", "radii_y", "radii_z"):
        assert np.array_equal(d[k], o[k]), k
    Hh.check_binning(d, o)
    if not precomp:
        assert _bitwise(d["cov3D"], o["cov3D"]), "the state's cov3D at modifier %g" % kw["scale_modifier"]
    vols, grads = {}, {}
    for chain in Hh.voxel_chains(n):
        label = "voxel %s %s %s" % (setting, grid, chain)
        vol, h, served = Hh.run_voxel_chain(chain, c, n, s, ctr, gpu, sticks_mode, **kw)
        vol2, h2, _ = Hh.run_voxel_chain(chain, c, n, s, ctr, gpu, sticks_mode, **kw)
        assert _bitwise(vol, vol2), label + ": two calls differ"
        vols[chain] = vol
        sp = Hh.parity_volume(oracle, o, vol, label)
        _assert_caps(label, sp, nvox)
        st = dict(counter=served, volume_max_rel_err=sp["max_rel_err"], volume_flip_candidates=sp["n_flip_candidates"] / nvox)
        if h is not None:
            assert h["num_rendered"] == d["num_rendered"]
            for k in ("radii_x", "radii_y", "radii_z", "tiles_touched", "point_list", "ranges"):
                assert np.array_equal(h[k], d[k]), (label, k)
            if precomp:
                _poison(gpu, 26 * P)
            gh = Hh.hip_voxel_backward(h, c, n, s, ctr, dL, gpu)
            gh2 = Hh.hip_voxel_backward(h2, c, n, s, ctr, dL, gpu)
            for k in VOXEL_GRADS:
                assert _bitwise(gh[k], gh2[k]), (label, k, "two calls differ")
            grads[chain] = gh
            sg = Hh.parity_voxel_grads(oracle, o, gh, c, dL, label, **kw)
            _assert_caps(label, sg)
            st.update(_grad_margins(VOXEL_GRADS, sg, label, precomp))
            assert sg["after_flips"]["max_err_over_tol_after_flips"] <= 0.3, (label, sg["after_flips"])
            if precomp:
                _assert_zero_rows(gh, P, label)
        if precomp:   # the modifier argument is dead under a precomputed covariance: forward and backward do not depend on it
            for other in (1.0, 1.9):
                vo, ho, _ = Hh.run_voxel_chain(chain, c, n, s, ctr, gpu, sticks_mode, scale_modifier=other,
                                               cov3D_precomp=kw["cov3D_precomp"])
                assert _bitwise(vo, vol), (label, "the volume depends on the modifier argument", other)
                if ho is not None:
                    go = Hh.hip_voxel_backward(ho, c, n, s, ctr, dL, gpu)
                    for k in VOXEL_GRADS:
                        assert _bitwise(go[k], gh[k]), (label, k, "depends on the modifier argument", other)
        Hh._log("optional_inputs", label, lambda: st)
        print(label, st)
    first = next(iter(vols))
    for chain in vols:
        assert _bitwise(vols[chain], vols[first]), "voxel %s %s: the volume of %s differs from %s" % (setting, grid, chain, first)
    first = next(iter(grads))
    for chain in grads:
        for k in VOXEL_GRADS:
            assert _bitwise(grads[chain][k], grads[first][k]), "voxel %s %s: %s of %s differs from %s" % (setting, grid, k, chain, first)
    # the geometry backward on the general chain's state where no production call leaves one (the 18-tile grid: small-grid
    # path and slab calls only): the debug call's
    if len(grads) < 2:
        label = "voxel %s %s general-debug" % (setting, grid)
        if precomp:
            _poison(gpu, 26 * P)
        gd = Hh.hip_voxel_backward(d, c, n, s, ctr, dL, gpu)
        sg = Hh.parity_voxel_grads(oracle, o, gd, c, dL, label, **kw)
        _assert_caps(label, sg)
        st = dict(counter=sv, **_grad_margins(VOXEL_GRADS, sg, label, precomp))
        assert sg["after_flips"]["max_err_over_tol_after_flips"] <= 0.3, (label, sg["after_flips"])
        if precomp:
            _assert_zero_rows(gd, P, label)
        Hh._log("optional_inputs", label, lambda: st)
        print(label, st)


# ------------------------------------------------------------------------------------------------ rasterizer, one view
def _lib():
    from r2_gaussian_amd import _lib as L
    return L.lib()


@pytest.fixture
def tile_first():
    """-> the setter of the tile-first chain's switch (0 off, 1 on, 2 forget this thread's predictions); switched on afterwards."""
    L = _lib()
    yield L.r2_tile_first_control
    L.r2_tile_first_control(1)


def _raster_chain(chain, c, v, gpu, tile_first, **kw):
    """One production forward on the named chain, asserted by its counter -> (state, counter increments)."""
    if chain == "general":
        tile_first(0)
        h, served = Hh.served(lambda: Hh.hip_raster(c, v, gpu, **kw))
        assert served == {"raster.general.switched_off": 1}, served
        assert not Hh.took_tile_first(h)
        return h, served
    tile_first(1)
    tile_first(2)
    Hh.hip_raster(c, v, gpu, **kw)                       # the first call of a size has nothing to predict from
    h, served = Hh.served(lambda: Hh.hip_raster(c, v, gpu, **kw))
    assert served.get("raster.tile_first") == 1 and not any(k.startswith("raster.general") for k in served), served
    assert Hh.took_tile_first(h)
    return h, served


@pytest.mark.parametrize("setting,beam", RASTER_CASES, ids=["%s-%s" % sb for sb in RASTER_CASES])
def test_rasterizer_both_chains(setting, beam, oracle, gpu, tile_first):
    c = _raster_cloud()
    n_rows = c.xyz.shape[0]
    kw = _inputs("raster", setting)
    precomp = kw["cov3D_precomp"] is not None
    npix = HW[0] * HW[1]
    for k in range(len(ANGLES)):
        v = _view(beam, k)
        o, dL, cond = _raster_oracle(setting, beam, k)
        Hh._log("optional_inputs", "raster %s %s view %d conditions" % (setting, beam, k), lambda: cond)
        d, sv = Hh.served(lambda: Hh.hip_raster(c, v, gpu, debug=True, **kw))
        assert sv == {"raster.general.debug": 1}, sv
        assert d["num_rendered"] == o["num_rendered"] > 0 and np.array_equal(d["radii"], o["radii"])
        Hh.check_binning(d, o)
        if not precomp:
            # the preprocess leaves before the covariance for a Gaussian behind the near plane (the reference too, its row is
            # then whatever the state buffer held): compared where the reference defines it
            front = oracle.mark_visible(c.xyz.numpy(), *Hh.np_view(v))
            assert 0 < (~front).sum() <= (o["radii"] == 0).sum()
            assert _bitwise(d["cov3D"][front], o["cov3D"][front]), "the state's cov3D at modifier %g" % kw["scale_modifier"]
        states = {}
        for chain in ("general", "tile-first"):
            label = "raster %s %s view %d %s" % (setting, beam, k, chain)
            h, served = _raster_chain(chain, c, v, gpu, tile_first, **kw)
            states[chain] = h
            assert h["num_rendered"] == o["num_rendered"]
            for f in ("radii", "point_list", "ranges"):
                assert np.array_equal(h[f], o[f]), (label, f)
            sp = Hh.parity_image(oracle, o, h["color"], label)
            _assert_caps(label, sp, npix)
            if precomp:
                _poison(gpu, 25 * n_rows)
            gh = Hh.hip_raster_backward(h, c, v, dL, gpu)
            sg = Hh.parity_raster_grads(oracle, o, gh, c, v, dL, label, **kw)
            _assert_caps(label, sg)
            st = dict(counter=served, image_max_rel_err=sp["max_rel_err"], image_flip_candidates=sp["n_flip_candidates"] / npix,
                      **_grad_margins(RASTER_GRADS, sg, label, precomp))
            if precomp:
                _assert_zero_rows(gh, n_rows, label)
            Hh._log("optional_inputs", label, lambda: st)
            print(label, st)
        a, b = states["general"], states["tile-first"]
        assert _bitwise(a["color"], b["color"]), "raster %s %s view %d: the chains' images differ" % (setting, beam, k)
        for f in ("radii", "point_list", "ranges"):
            assert np.array_equal(a[f], b[f]), f


# ------------------------------------------------------------------------------------------------ rasterizer, batched views
def _batch(c, views, dev, scale_modifier=1.0, cov3D_precomp=None):
    from r2_gaussian_amd import _C
    e = torch.empty(0)
    vm = torch.stack([v.world_view_transform for v in views]).to(dev)
    pm = torch.stack([v.full_proj_transform for v in views]).to(dev)
    v0 = views[0]
    sc, q = (c.scales.to(dev), c.rotations.to(dev)) if cov3D_precomp is None else (e, e)
    cp = e if cov3D_precomp is None else torch.as_tensor(cov3D_precomp).to(dev)
    args = (c.xyz.to(dev), c.density.to(dev), sc, q, scale_modifier, cp, vm, pm, v0.tanfovx, v0.tanfovy, v0.image_height,
            v0.image_width, v0.mode, False)
    out = _C.rasterize_gaussians_batch(*args)
    torch.cuda.synchronize()
    return args, out


def _batch_backward(args, out, dL):
    from r2_gaussian_amd import _C
    R, _color, radii, gb, bb, ib = out
    res = _C.rasterize_gaussians_backward_batch(args[0], radii, args[2], args[3], args[4], args[5], args[6], args[7], args[8],
                                                args[9], dL, gb, R, bb, ib, args[12], False)
    torch.cuda.synchronize()
    return {n: t.cpu().numpy() for n, t in zip(RASTER_GRADS, res)}


@pytest.mark.parametrize("chain", ["tile-first", "general"])
@pytest.mark.parametrize("setting", list(SETTINGS))
def test_rasterizer_batched_views(setting, chain, oracle, gpu, tile_first):
    """V = 3: the multi-view geometry backward indexes a caller's covariance per Gaussian and the state's per view instance."""
    c = _raster_cloud()
    n_rows = c.xyz.shape[0]
    V = len(ANGLES)
    kw = _inputs("raster", setting)
    precomp = kw["cov3D_precomp"] is not None
    views = [_view("cone", k) for k in range(V)]
    tile_first(1 if chain == "tile-first" else 0)
    tile_first(2)
    _batch(c, [S.make_view(0.1 + 0.7 * k, HW) for k in range(V)], gpu, **kw)      # first batched call of this size
    (args, out), served = Hh.served(lambda: _batch(c, views, gpu, **kw))           # the second: predicted / hinted
    want = "raster.tile_first" if chain == "tile-first" else "raster.general.switched_off"
    assert served.get(want) == 1 and (chain == "general" or not any(k.startswith("raster.general") for k in served)), served
    R, color, radii, _gb, _bb, _ib = out
    assert color.shape == (V,) + HW and radii.shape == (V, n_rows)
    singles = [Hh.hip_raster(c, v, gpu, **kw) for v in views]
    assert R == sum(h["num_rendered"] for h in singles)
    for k, h in enumerate(singles):
        assert np.array_equal(radii[k].cpu().numpy(), h["radii"]), "radii of view %d" % k
        assert _bitwise(color[k].cpu().numpy(), h["color"][0]), "image of view %d is not bit-identical" % k
    g = torch.Generator().manual_seed(3)
    dL = ((torch.rand((V,) + HW, generator=g) * 2 - 1) / float(HW[0] * HW[1])).to(gpu)
    if precomp:
        _poison(gpu, 8 * V * n_rows + 17 * n_rows)
    gh = _batch_backward(args, out, dL)
    assert gh["dL_dmeans2D"].shape == (V, n_rows, 3) and gh["dL_dmu"].shape == (V, n_rows)
    summed = ("dL_dopacity", "dL_dmeans3D", "dL_dcov3D", "dL_dscales", "dL_drotations")
    tot = {n: 0.0 for n in summed}
    per_view = []
    for k, (v, h) in enumerate(zip(views, singles)):
        gs = Hh.hip_raster_backward(h, c, v, dL[k:k + 1].cpu().numpy(), gpu)
        per_view.append(gs)
        assert _bitwise(gh["dL_dmeans2D"][k], gs["dL_dmeans2D"]), "dL_dmeans2D of view %d" % k
        assert _bitwise(gh["dL_dmu"][k], gs["dL_dmu"].reshape(-1)), "dL_dmu of view %d" % k
        for n in summed:
            tot[n] = tot[n] + gs[n].astype(np.float64)
    worst = {}
    for n in summed:
        if precomp and n in GEOM_ONLY:
            continue
        scale = float(np.abs(tot[n]).max())
        assert scale > 0, n
        worst[n] = float(np.abs(gh[n] - tot[n]).max()) / scale
        assert worst[n] <= 2e-6, (n, worst[n])   # same terms, summed in one kernel instead of V
    if precomp:
        _assert_zero_rows(gh, n_rows, "batch %s %s" % (setting, chain))
    st = dict(counter=served, sum_over_views_err_over_scale=worst)
    for k in (0, 2):   # against the oracle, with the setting passed through
        label = "raster batch %s %s view %d" % (setting, chain, k)
        o, _dL, _cond = _raster_oracle(setting, "cone", k)
        sp = Hh.parity_image(oracle, o, color[k:k + 1].cpu().numpy(), label)
        _assert_caps(label, sp, HW[0] * HW[1])
        sg = Hh.parity_raster_grads(oracle, o, per_view[k], c, views[k], dL[k:k + 1].cpu().numpy(), label, **kw)
        _assert_caps(label, sg)
        st["view %d" % k] = _grad_margins(RASTER_GRADS, sg, label, precomp)
    Hh._log("optional_inputs", "raster batch %s %s" % (setting, chain), lambda: st)
    print("raster batch", setting, chain, st)


# ------------------------------------------------------------------------------------------------ the modules
def _raster_settings(views, dev, mod):
    from r2_gaussian_amd import GaussianRasterizationSettings
    v0 = views[0]
    st = lambda f: (torch.stack([f(v) for v in views]) if len(views) > 1 else f(v0)).to(dev)   # noqa: E731
    return GaussianRasterizationSettings(HW[0], HW[1], v0.tanfovx, v0.tanfovy, mod, st(lambda v: v.world_view_transform),
                                         st(lambda v: v.full_proj_transform), st(lambda v: v.camera_center), False, v0.mode, False)


def test_rasterizer_modules_with_a_covariance_leaf(gpu, tile_first):
    from r2_gaussian_amd import GaussianRasterizer, GaussianRasterizerBatch
    from r2_gaussian_amd.rasterization import rasterize_gaussians
    c = _raster_cloud()
    n_rows = c.xyz.shape[0]
    kw = _inputs("raster", "precomp")
    tile_first(0)   # one chain for the module's call and the direct one
    xyz, rho = c.xyz.to(gpu), c.density.to(gpu)
    # one view
    v = _view("cone", 1)
    dL = S.make_pixel_grad(*HW, seed=5)
    h = Hh.hip_raster(c, v, gpu, **kw)
    want = Hh.hip_raster_backward(h, c, v, dL.numpy(), gpu)
    cov = torch.as_tensor(kw["cov3D_precomp"]).to(gpu).requires_grad_(True)
    m2 = torch.zeros((n_rows, 3), device=gpu, requires_grad=True)
    img, radii = GaussianRasterizer(_raster_settings([v], gpu, kw["scale_modifier"]))(
        means3D=xyz, means2D=m2, opacities=rho, cov3D_precomp=cov)
    assert _bitwise(img.detach().cpu().numpy(), h["color"]) and np.array_equal(radii.cpu().numpy(), h["radii"])
    img.backward(dL.to(gpu))
    assert cov.grad is not None and _bitwise(cov.grad.cpu().numpy(), want["dL_dcov3D"])
    assert np.abs(want["dL_dcov3D"]).max() > 0
    # ... the absent scales and rotations get no gradient (the functional form, with empty leaves in their places)
    e_s, e_q = (torch.empty(0, requires_grad=True) for _ in range(2))
    cov2 = cov.detach().clone().requires_grad_(True)
    img2, _ = rasterize_gaussians(xyz, torch.zeros((n_rows, 3), device=gpu, requires_grad=True), rho, e_s, e_q, cov2,
                                  _raster_settings([v], gpu, kw["scale_modifier"]))
    img2.backward(dL.to(gpu))
    assert e_s.grad is None and e_q.grad is None and torch.equal(cov2.grad, cov.grad)
    # V views
    views = [_view("cone", k) for k in range(len(ANGLES))]
    V = len(views)
    g = torch.Generator().manual_seed(9)
    dLb = ((torch.rand((V,) + HW, generator=g) * 2 - 1) / float(HW[0] * HW[1])).to(gpu)
    args, out = _batch(c, views, gpu, **kw)
    wantb = _batch_backward(args, out, dLb)
    covb = cov.detach().clone().requires_grad_(True)
    m2b = torch.zeros((V, n_rows, 3), device=gpu, requires_grad=True)
    imgb, _ = GaussianRasterizerBatch(_raster_settings(views, gpu, kw["scale_modifier"]))(
        means3D=xyz, means2D=m2b, opacities=rho, cov3D_precomp=covb)
    assert _bitwise(imgb.detach().cpu().numpy(), out[1].cpu().numpy())
    imgb.backward(dLb)
    assert covb.grad is not None and _bitwise(covb.grad.cpu().numpy(), wantb["dL_dcov3D"])
    assert np.abs(wantb["dL_dcov3D"]).max() > 0 and _bitwise(m2b.grad.cpu().numpy(), wantb["dL_dmeans2D"])


def test_voxelize_gaussians_with_a_covariance_leaf(gpu):
    """The functional form takes what the ABI requires: scales, empty rotations and the covariance."""
    from r2_gaussian_amd import GaussianVoxelizationSettings
    from r2_gaussian_amd.voxelization import voxelize_gaussians
    c = _voxel_cloud()
    n, s, ctr = GRID_LARGE
    kw = _inputs("voxel", "precomp")
    dL = _voxel_dL(n)
    h = Hh.hip_voxel(c, n, s, ctr, gpu, **kw)
    want = Hh.hip_voxel_backward(h, c, n, s, ctr, dL, gpu)
    vs = GaussianVoxelizationSettings(kw["scale_modifier"], n[0], n[1], n[2], s[0], s[1], s[2], ctr[0], ctr[1], ctr[2], False, False)
    cov = torch.as_tensor(kw["cov3D_precomp"]).to(gpu).requires_grad_(True)
    sc = c.scales.to(gpu).requires_grad_(True)
    e_q = torch.empty(0, requires_grad=True)
    vol, (rx, _ry, _rz) = voxelize_gaussians(c.xyz.to(gpu), c.density.to(gpu), sc, e_q, cov, vs)
    assert _bitwise(vol.detach().cpu().numpy(), h["vol"]) and np.array_equal(rx.cpu().numpy(), h["radii_x"])
    vol.backward(torch.as_tensor(dL).to(gpu))
    assert cov.grad is not None and _bitwise(cov.grad.cpu().numpy(), want["dL_dcov3D"])
    assert np.abs(want["dL_dcov3D"]).max() > 0
    assert e_q.grad is None                                  # absent: no gradient
    assert sc.grad is None or not sc.grad.any()              # passed for the radii only: nothing flows into them


def test_voxelizer_module_refuses_a_covariance_without_scales(gpu):
    """GaussianVoxelizer(...)(cov3D_precomp=...) passes empty scales, as the reference's module does; the reference then
    dereferences them for the radii (VOX/forward.cu:137-143).  Here the call is refused before anything is launched, and the
    process goes on."""
    from r2_gaussian_amd import GaussianVoxelizationSettings, GaussianVoxelizer, _C
    from r2_gaussian_amd._lib import R2HipError
    c = _voxel_cloud()
    n, s, ctr = GRID_SMALL
    kw = _inputs("voxel", "precomp")
    vs = GaussianVoxelizationSettings(kw["scale_modifier"], n[0], n[1], n[2], s[0], s[1], s[2], ctr[0], ctr[1], ctr[2], False, False)
    xyz, rho = c.xyz.to(gpu), c.density.to(gpu)
    cov = torch.as_tensor(kw["cov3D_precomp"]).to(gpu)
    with pytest.raises(R2HipError, match="scales are required"):
        GaussianVoxelizer(vs)(means3D=xyz, opacities=rho, cov3D_precomp=cov)
    # the same call at the C ABI, on outputs of our own: nothing was launched, they stay as they were
    out = torch.full(n, 7.0, device=gpu)
    radii = torch.full((3, P), 7, dtype=torch.int32, device=gpu)
    torch.cuda.synchronize()
    with pytest.raises(R2HipError, match="scales are required"):
        _C._forward("r2_voxel_forward_slab", gpu, _C._hooks(gpu), P, n[0], n[1], n[2], float(s[0]), float(s[1]), float(s[2]),
                    float(ctr[0]), float(ctr[1]), float(ctr[2]), 0, (n[0] + 7) // 8, xyz, rho, None, float(kw["scale_modifier"]),
                    None, cov, 0, out, radii[0], radii[1], radii[2], 0)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((radii == 7).all())
    # ... and the next call runs
    vol, _ = GaussianVoxelizer(vs)(means3D=xyz, opacities=rho, scales=c.scales.to(gpu), rotations=c.rotations.to(gpu))
    h = Hh.hip_voxel(c, n, s, ctr, gpu, scale_modifier=kw["scale_modifier"])
    assert _bitwise(vol.cpu().numpy(), h["vol"]) and float(vol.max()) > 0
