"""GPU: every voxelizer render chain against the float64 restatement (tests/voxel_ref.py) on scenes at the edges of its tiers
(tests/voxel_scenes.py): needles and pancakes on both sides of needs_exact_slab3, sub-voxel Gaussians, peak densities at and
around the 1e-6 cut-off and up to 50, anisotropic voxels on a grid one voxel thick, centres outside the volume / on voxel
centres / on tile boundaries, and tile lists of every length.

The reference takes the record and the lists of a debug call (both pinned to the oracle by tests/test_voxel_gpu.py); the volumes
come from production calls of each chain that can serve the grid -- the small-grid path (<= 64 tiles), the general chain's
production render through x-slab calls of <= 64 tiles, the stick-first and the general chain (r2_voxel_sticks_control) on larger
grids -- and r2_path_stats shows which chain served each call.  Every voxel must lie within the float64 bound, dL/dopacity within
its own, dL/dmeans3D within its own; the other gradients meet the oracle parity of the existing voxel tests (GRAD_PARITY_SCENES)
or a float64 arbiter (ARBITER_KEYS); the lists equal the oracle's; two calls are bit-identical."""
import numpy as np
import pytest
import torch

from tests import helpers as Hh
from tests import voxel_ref as VR
from tests import voxel_scenes as VS

pytestmark = pytest.mark.gpu

GRAD_KEYS = ("dL_dopacity", "dL_dmeans3D", "dL_dcov3D", "dL_dscales", "dL_drotations")
# Scenes whose means / covariance / scale / rotation gradients are also held to the oracle parity of tests/test_voxel_gpu.py
# (<= 2e-4 of the scale unflagged, after flips <= 0.3).  On the other three, the float64 arbiter below (the render's sums in
# float64 through the geometry chain's Jacobian) shows who is off at the elements outside that parity's tolerance, in units of it:
#   faces (dL_dscales, 32^3): kernel 0.74, oracle 0.96, kernel - oracle 1.37 -- the oracle's float32 sums, not the kernel;
#   tier (needles, pancakes; dL_dscales, dL_drotations): kernel 2436 / 2.6, oracle 3200 / 3.1, and the float32 chain applied to
#     the float64 sums 3730 / 3.6 -- the chain of an ill-conditioned covariance, the same in both, not the render;
#   subvoxel (dL_dmeans3D, dL_dscales): kernel 39 / 1.4, oracle 0.25 / 0.89 -- the kernel's moment form (conic . sum w d)
#     loses what the per-pair form keeps where conic . d cancels; dL_dmeans3D is held to the float64 bound of that form instead.
GRAD_PARITY_SCENES = ("opacity", "aniso", "lists")
# ... and what is held to the float64 arbiter, per scene (dL_dopacity and dL_dmeans3D: float64 bounds on every scene)
ARBITER_KEYS = {"tier": ("dL_dcov3D",), "subvoxel": ("dL_dcov3D", "dL_drotations"),
                "faces": ("dL_dcov3D", "dL_dscales", "dL_drotations")}


_served = Hh.served


def _dL(n, seed):
    g = torch.Generator().manual_seed(seed)
    return ((torch.rand(*n, generator=g) * 2 - 1) / float(np.prod(n))).numpy()


def _reference(h, n, voxels=None, dL=None, s=None):
    return VR.render(h["means3D_norm"], h["conic"], h["rec"][:, 3], h["point_list"], h["ranges"], n, voxels=voxels, dL=dL,
                     sVoxel=s)


def _arbiter(oracle, o, gh, c, dL, ref, keys):
    """Geometry gradients against the float64 render sums carried through the chain's Jacobian (the oracle's, column by column,
    as oracle/parity.py builds it), within that parity's tolerance |J| (1e-4 sum|terms| + flip budget + 1e-6 |sum|).
    -> {key: worst err / tol}."""
    S, A, F = oracle.voxel_backward_audit(o, dL)
    P = o["P"]
    sc, rot = c.scales.numpy(), c.rotations.numpy()
    f64 = {k: 0.0 for k in keys}
    tol = {k: 0.0 for k in keys}
    for q in range(9):
        unit = np.zeros((P, 10), np.float32)
        unit[:, q] = 1.0
        J = oracle.voxel_geom_chain(o, unit, sc, rot, 1.0, None)
        for k in keys:
            Jq = J[k].astype(np.float64)
            f64[k] = f64[k] + Jq * ref["raw"][:, q:q + 1]
            tol[k] = tol[k] + np.abs(Jq) * (1e-4 * A[:, q:q + 1] + F[:, q:q + 1] + 1e-6 * np.abs(S[:, q:q + 1]))
    out = {}
    for k in keys:
        e = np.abs(np.asarray(gh[k], np.float64).reshape(f64[k].shape) - f64[k])
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(tol[k] > 0, e / tol[k], np.where(e == 0, 0.0, np.inf))
        out[k] = float(r.max())
    return out


def _same_lists(h, d):
    assert h["num_rendered"] == d["num_rendered"]
    assert np.array_equal(h["point_list"], d["point_list"]) and np.array_equal(h["ranges"], d["ranges"])


def _bitwise(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


# ------------------------------------------------------------------------------------------------ what each scene must hold
def _instance_tiers(d):
    """-> (exact flag per listed instance, tile of each instance): needs_exact_slab3 restated on the debug record."""
    rec = VR.record(d["means3D_norm"], d["conic"], d["rec"][:, 3])
    exact = VR.needs_exact(rec)
    return exact[d["point_list"]], d["tiles"], rec


def _assert_coverage(name, sc, n, s, d, ref):
    vis = d["tiles_touched"] > 0
    if name == "tier":
        ex, tiles, _ = _instance_tiers(d)
        n_ex, n_st = int(ex.sum()), int((~ex).sum())
        assert n_ex >= 100 and n_st >= 100, ("instances exact / stepped", n_ex, n_st)
        both = np.bincount(tiles[ex], minlength=len(d["ranges"])) * np.bincount(tiles[~ex], minlength=len(d["ranges"]))
        assert (both > 0).any(), "no tile list holds entries of both tiers"
        return dict(exact=n_ex, stepped=n_st, mixed_lists=int((both > 0).sum()))
    if name == "subvoxel":
        sig = sc.cloud.scales.numpy() / (np.array(s) / np.array(n))
        assert sig.min() >= 0.049 and sig.max() <= 0.41
        dead = vis & (ref["dop_pairs"] == 0)
        assert dead.sum() >= 50, "sub-voxel Gaussians that reach no voxel centre above the cut-off: %d" % dead.sum()
        return dict(visible=int(vis.sum()), no_live_pair=int(dead.sum()))
    if name == "opacity":
        op = d["rec"][:, 3]
        near = vis & (np.abs(op / 1e-6 - 1.0) <= 0.01)
        below = vis & (op < 1e-6) & ~near
        high = vis & (op >= 1.0)
        assert near.sum() >= 50 and below.sum() >= 50 and high.sum() >= 10, (near.sum(), below.sum(), high.sum())
        assert int(ref["n_band"].sum()) > 0, "no pair on the cut-off"
        return dict(near_cutoff=int(near.sum()), below_cutoff=int(below.sum()), above_one=int(high.sum()),
                    band_pairs=int(ref["n_band"].sum()))
    if name == "aniso":
        dv = np.array(s) / np.array(n)
        assert min(n) == 1 and abs(dv.max() / dv.min() - 8.0) < 1e-6
        return dict(voxel=tuple(float(v) for v in dv))
    if name == "faces":
        pv = d["means3D_norm"].astype(np.float64)
        outside = vis & ((pv < 0) | (pv > np.array(n))).any(1)
        on_centre = vis & (pv - 0.5 == np.floor(pv)).all(1)
        on_tile = vis & (np.mod(pv, 8.0) == 0).all(1)
        assert outside.sum() >= 100 and on_centre.sum() >= 100 and on_tile.sum() >= 20, (outside.sum(), on_centre.sum(), on_tile.sum())
        return dict(outside=int(outside.sum()), on_voxel_centre=int(on_centre.sum()), on_tile_corner=int(on_tile.sum()))
    if name == "lists":
        ln = (d["ranges"][:, 1].astype(np.int64) - d["ranges"][:, 0])
        assert ((ln > 0) & (ln < 25)).any() and (ln > 256).any(), (ln.min(), ln.max())
        # a wave's remainder under VFWD_STEP_MIN (6) at the flush: lists of 25..128 are one work item on every chain; the
        # stepped entries live in a slab are consumed 64 at a time, the rest (count mod 64) is flushed voxel-parallel
        ex, tiles, rec = _instance_tiers(d)
        gx, gy = (n[0] + 7) // 8, (n[1] + 7) // 8
        flushes = 0
        for t in np.nonzero((ln >= 25) & (ln <= 128))[0]:
            a, b = d["ranges"][t]
            ids = d["point_list"][a:b]
            sub = {k: v[ids] for k, v in rec.items()}
            tx, ty, tz = t % gx, (t // gx) % gy, t // (gx * gy)
            for sl in range(8):
                live = VR.slab_live(sub, tx * 8 + sl + 0.5, ty * 8.0, tz * 8.0) & ~ex[a:b]
                flushes += int(1 <= live.sum() % 64 <= 5)
        assert flushes > 0, "no slab ends with a voxel-parallel flush"
        return dict(shortest=int(ln[ln > 0].min()), longest=int(ln.max()), short_lists=int(((ln > 0) & (ln < 25)).sum()),
                    long_lists=int((ln > 256).sum()), flush_slabs=flushes)
    raise KeyError(name)


# ------------------------------------------------------------------------------------------------ the chains
sticks_mode = pytest.fixture(Hh.sticks_mode)


_chains = Hh.voxel_chains
_run_chain = Hh.run_voxel_chain


@pytest.mark.parametrize("name", list(VS.SCENES))
def test_every_chain_within_the_float64_bound(name, oracle, gpu, sticks_mode):
    sc = VS.SCENES[name]()
    c = sc.cloud
    assert c.xyz.shape[0] <= 20000
    for gi, (n, s, ctr) in enumerate(sc.grids):
        grid = "x".join(map(str, n))
        d = Hh.hip_voxel(c, n, s, ctr, gpu, debug=True)   # the records and lists (debug mode renders with its own kernel)
        assert d["num_rendered"] > 0
        dL = _dL(n, 7 + gi)
        ref = _reference(d, n, dL=dL, s=s)
        o = Hh.oracle_voxel(oracle, c, n, s, ctr)
        # the lists the reference is built on are the oracle's, bit for bit, on these scenes too
        assert d["num_rendered"] == o["num_rendered"]
        for k in ("radii_x", "radii_y", "radii_z"):
            assert np.array_equal(d[k], o[k]), k
        Hh.check_binning(d, o)
        tight, nonempty = VR.tightness(ref)
        tight_dop, n_dop = VR.tightness_dop(ref)
        cov = _assert_coverage(name, sc, n, s, d, ref)
        Hh._log("voxel_tiers", "%s %s coverage" % (name, grid), lambda: dict(cov, tightness=tight, nonempty_voxels=nonempty,
                                                                                 dop_tightness=tight_dop, gaussians=n_dop))
        assert tight >= 0.95, "%s %s: the bound is below the smallest contribution in only %.3f of %d voxels" % (
            name, grid, tight, nonempty)
        if name == "subvoxel":
            # few pairs per Gaussian: the dL/dopacity bound is below the smallest single term, so a dropped or doubled
            # backward item shows (elsewhere a Gaussian has hundreds of pairs and gamma_m sum|w| outgrows its smallest one)
            assert tight_dop >= 0.95, (name, grid, tight_dop, n_dop)
        for chain in _chains(n):
            label = "%s %s %s" % (name, grid, chain)
            vol, h, _ = _run_chain(chain, c, n, s, ctr, gpu, sticks_mode)
            vol2, h2, _ = _run_chain(chain, c, n, s, ctr, gpu, sticks_mode)
            assert _bitwise(vol, vol2), label + ": two calls differ"
            worst = VR.check(vol, ref, label)
            st = dict(worst_err_over_bound=worst)
            if h is not None:
                _same_lists(h, d)
                gh = Hh.hip_voxel_backward(h, c, n, s, ctr, dL, gpu)
                gh2 = Hh.hip_voxel_backward(h2, c, n, s, ctr, dL, gpu)
                for k in GRAD_KEYS:
                    assert _bitwise(gh[k], gh2[k]), (label, k, "two calls differ")
                st["dop_worst_err_over_bound"] = VR.check_dop(gh["dL_dopacity"], ref, label)
                st["dmean_worst_err_over_bound"] = VR.check_dmean(gh["dL_dmeans3D"], ref, label)
                if name in ARBITER_KEYS:
                    arb = _arbiter(oracle, o, gh, c, dL, ref, ARBITER_KEYS[name])
                    st["arbiter_worst_err_over_tol"] = arb
                    assert max(arb.values()) <= 1.0, (label, arb)
                if name in GRAD_PARITY_SCENES:
                    sg = Hh.parity_voxel_grads(oracle, o, gh, c, dL, label)
                    for k in GRAD_KEYS:
                        assert sg[k]["max_err_over_scale_unflagged"] <= 2e-4, (label, k, sg[k])
                    assert sg["after_flips"]["max_err_over_tol_after_flips"] <= 0.3, (label, sg["after_flips"])
            Hh._log("voxel_tiers", label, lambda: st)
            print(label, st)


def test_256_cubed_sampled_on_both_chains_and_in_x_slabs(oracle, gpu, sticks_mode):
    sc = VS.big_scene()
    c = sc.cloud
    (n, s, ctr), = sc.grids
    d = Hh.hip_voxel(c, n, s, ctr, gpu, debug=True)
    Hh.check_binning(d, Hh.oracle_voxel(oracle, c, n, s, ctr, render=False))
    # ~1e5 voxels, seeded, from the tiles that hold a list
    rng = np.random.default_rng(11)
    ln = d["ranges"][:, 1].astype(np.int64) - d["ranges"][:, 0]
    live_tiles = np.nonzero(ln > 0)[0]
    t = rng.choice(live_tiles, 100000)
    loc = rng.integers(0, 8, (100000, 3))
    gx, gy = n[0] // 8, n[1] // 8
    x, y, z = (t % gx) * 8 + loc[:, 0], ((t // gx) % gy) * 8 + loc[:, 1], (t // (gx * gy)) * 8 + loc[:, 2]
    vox = np.unique((x * n[1] + y) * n[2] + z)
    ref = _reference(d, n, voxels=vox)
    tight, nonempty = VR.tightness(ref)
    assert nonempty > 20000 and tight >= 0.95, (tight, nonempty)
    ex, _, _ = _instance_tiers(d)
    assert ex.sum() >= 100 and (~ex).sum() >= 100
    for chain in ("sticks", "general"):
        vol, h, _ = _run_chain(chain, c, n, s, ctr, gpu, sticks_mode)
        _same_lists(h, d)
        worst = VR.check(vol.reshape(-1)[vox], ref, "256^3 " + chain)
        Hh._log("voxel_tiers", "big256 %s" % chain, lambda: dict(worst_err_over_bound=worst, voxels=int(vox.size), tightness=tight))
        print("big256", chain, worst)
    sticks_mode(1)
    vx = vox // (n[1] * n[2])
    for t0, t1 in ((0, 11), (11, 22), (22, 32)):
        h, served = _served(lambda: Hh.hip_voxel(c, n, s, ctr, gpu, slab=(t0, t1)))
        assert served == {"voxel.stick_first": 1}, served
        sel = (vx >= 8 * t0) & (vx < 8 * t1)
        sub = {k: (v[sel] if isinstance(v, np.ndarray) and v.shape[:1] == vox.shape else v) for k, v in ref.items()}
        local = vox[sel] - 8 * t0 * n[1] * n[2]
        worst = VR.check(h["vol"].reshape(-1)[local], sub, "256^3 slab %d-%d" % (t0, t1))
        Hh._log("voxel_tiers", "big256 slab %d-%d" % (t0, t1), lambda: dict(worst_err_over_bound=worst))
        print("big256 slab", t0, t1, worst)
