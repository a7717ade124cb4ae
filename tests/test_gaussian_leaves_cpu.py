"""CPU: the leaf-culled exact line integrals (tests/gaussian_leaves_ref.py): the measured float32 error the GPU tolerance is
taken from, the three C symbols, cloud_order, the float32 restatement of the prepare kernel and the leaf test against the
pairs the rule sums, what the ordering buys, and the stochastic refinement loop on the host."""
import os
import re

import numpy as np
import pytest
import torch

from tests import gaussian_bundle_ref as B
from tests import gaussian_leaves_ref as LR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("r2_integrate_gaussians_leaves", "r2_integrate_gaussians_leaves_backward", "r2_integrate_gaussians_leaves_workspace_bytes")


def test_stored_e32_matches_a_fresh_measurement():
    """tests/golden/gaussian_leaves/e32.json (python -m tests.gaussian_leaves_ref) within 10 % of a fresh measurement, the
    tolerance tests/test_gaussian_bundle_cpu.py uses for its file."""
    stored = LR.load_e32()
    assert sorted(stored) == sorted(LR.SCENES)
    for name in LR.SCENES:
        fresh = LR.measure_e32(name)
        assert sorted(fresh) == sorted(stored[name])
        for k, v in fresh.items():
            assert abs(stored[name][k] - v) <= 0.1 * v, (name, k, stored[name][k], v)


def test_symbols_are_declared_and_exported_and_the_abi_is_3():
    from r2_gaussian_amd import _lib
    with open(os.path.join(ROOT, "include", "r2hip.h")) as f:
        header = f.read()
    assert re.search(r"#define\s+R2_ABI_VERSION\s+3\b", header) and _lib.R2_ABI_VERSION == 3
    L = _lib.lib()
    assert L.r2_abi_version() == 3
    for name in SYMBOLS:
        assert re.search(r"R2_API\s+\w+\s+%s\(" % name, header), name
        assert name in _lib.exported_symbols() and hasattr(L, name), name
    # host-only: 80 bytes per Gaussian and 24 per leaf of 64, nothing without rays or without a cloud
    ws = L.r2_integrate_gaussians_leaves_workspace_bytes
    assert ws(0, 100) == 0 and ws(100, 0) == 0
    for P in (1, 63, 64, 65, 129, 1500, 1 << 29):
        assert ws(1, P) == 80 * P + 24 * ((P + 63) // 64), P


def test_cloud_order():
    """A permutation, the same on every call, rows with a non-finite mean or scale (or no positive scale) first, large
    Gaussians before small ones; it accepts an empty cloud and one whose means coincide."""
    from r2_gaussian_amd.gaussian_projector import cloud_order
    xyz, _, sc, _ = (torch.from_numpy(a.copy()) for a in LR._mixed())
    xyz[7, 1], xyz[900, 0], sc[33, 2] = float("nan"), float("inf"), float("nan")
    sc[1201] = -1.0
    perm = cloud_order(xyz, sc)
    P = xyz.shape[0]
    assert perm.dtype == torch.int64 and perm.shape == (P,) and torch.equal(torch.sort(perm)[0], torch.arange(P))
    assert torch.equal(perm, cloud_order(xyz, sc)) and torch.equal(perm, cloud_order(xyz.clone(), sc.clone(), 1.0))
    assert perm[:4].tolist() == [7, 33, 900, 1201]
    big = sc.amax(1)[perm[4:]]
    assert big[:25].min() > 4.0 * big[40:].max()   # the 30 enlarged Gaussians (those not spoilt above) lead
    assert cloud_order(xyz[:0], sc[:0]).shape == (0,)
    same = torch.zeros((5, 3))
    assert torch.equal(cloud_order(same, same + 0.1), torch.arange(5))
    assert torch.equal(cloud_order(same, same), torch.arange(5))   # no positive scale anywhere


@pytest.mark.parametrize("name", ["spread", "spread_ordered", "mixed", "tiny", "offset_tiny", "singular", "inside"])
def test_no_summed_pair_is_culled(name):
    """The float32 restatement of the prepare kernel (gauss_radius, the leaf boxes) and of the leaf test (the slab test with
    its allowances), in the header's operation order: every pair that the rule sums in float32 belongs to a Gaussian with
    radius >= 0 whose leaf the ray's test keeps."""
    sc = LR.scene(name) if name in LR.SCENES else B.scene(name)
    summed, culled, share = LR.culled_summed_pairs(sc)
    print("%s: %d summed pairs, %d culled, %.3f of the (ray, leaf) pairs met" % (name, summed, culled, share))
    assert summed > 300 and culled == 0


def test_ordering_culls():
    """scene.make_cloud(50000) with 2 % of the Gaussians 20 x larger, 400 random lines through the cloud: under cloud_order
    a line meets at most half of the leaves (the ordering of DESIGN.md section 4's table gives 0.28 for leaves of 64, and 0.42
    even for leaves of 256); in index order it meets them all."""
    from r2_gaussian_amd import scene as S
    from r2_gaussian_amd.gaussian_projector import cloud_order
    c = S.make_cloud(50000, seed=7)
    scales = c.scales.clone()
    scales[torch.from_numpy(np.random.RandomState(8).permutation(50000)[:1000])] *= 20.0
    o, d = B._lines(400, 9, half=0.5, past=0.0)
    share = {}
    for which, perm in (("index", torch.arange(50000)), ("ordered", cloud_order(c.xyz, scales))):
        cloud = tuple(t[perm].contiguous().numpy() for t in (c.xyz, c.density, scales, c.rotations))
        lo, hi = LR.leaf_boxes32(cloud[0], LR.radius32(*cloud))
        share[which] = float(LR.rays_meet_leaves32(o, d, False, lo, hi).mean())
    print("share of (line, leaf) pairs met: index order %.3f, cloud_order %.3f" % (share["index"], share["ordered"]))
    assert share["ordered"] <= 0.5 and share["index"] > 0.99


def test_stochastic_refinement_converges_on_the_host():
    """refine_geometry(rays_per_step=REFINE_RAYS, seed=REFINE_SEED)'s loop in float64 on the host, a quarter of the pixels per
    step: the final offset error is below half the initial one, the criterion of the float64 loop over whole views.  With
    every pixel per step the loop is that float64 loop up to the association of the loss."""
    from tests import gaussian_project_rays_ref as Q
    gold, st = Q.load_refine(), Q.refine_setup()
    assert LR.REFINE_RAYS == (3 * st["H"] * st["W"]) // 4
    true = np.asarray(gold["true_offDetector"])
    p, hist = LR.refine_host_subset(st, gold["K"], gold["lr"])
    err = float(np.abs(p - true).max())
    print("quarter of the pixels: offDetector %s, error %.3e of initially %.3e, loss %.3e -> %.3e" % (p, err, gold["initial_error64"], hist[0], hist[-1]))
    assert err < 0.5 * gold["initial_error64"]
    p, _ = LR.refine_host_subset(st, gold["K"], gold["lr"], rays_per_step=3 * st["H"] * st["W"])
    assert np.abs(p - np.asarray(gold["final64"])).max() <= 1e-12


def test_one_pair_has_one_pair_per_ray_and_no_exactly_cancelled_component():
    """Every line of `one_pair` sums exactly one pair in float32, and no gradient component has a float64 sum of
    |contributions| under FLOOR where the float32 restatement is non-zero: the bracket of the GPU test, which is absolute
    there, then holds nobody's rounding noise against the underflow floor."""
    r = LR.reference("one_pair")
    sc = r["scene"]
    summed = LR.summed32(sc["origins"], sc["directions"], sc["half_line"], *sc["cloud"])
    assert (summed.sum(1) == 1).all() and summed.shape == (300, 700)
    f32 = LR.bundle32(sc["origins"], sc["directions"], sc["half_line"], *sc["cloud"], mod=sc["mod"], G=sc["G"])
    for k in B.GRADS:
        assert not ((r["hi"]["gabs"][k] <= B.FLOOR) & (f32["grads"][k] != 0)).any(), k
