"""tests/densify_ref.py, the float64 statement of densify_and_prune with its per-element error bounds, checked on the CPU before
any kernel is held against it (tests/test_densify_edges_gpu.py):

* against the fixtures written by the reference's own GaussianModel.densify_and_prune (tests/golden/train/densify_{A,B,C}.npz);
* against the torch statement (mini_trainer.Model.densify_and_prune, float32, the reference's operations in the reference's
  order) on the edge scene -- this is where the NaN, inf and on-threshold conventions are settled by the reference's code;
* the bound is honest and not vacuous: an independent float32 evaluation in the kernel's operation order (numpy, no fused
  operations) stays within it, and comes close to it.  Worst error / bound measured over the edge scenes at P = 257 and 4097
  (test_the_bound_is_honest_and_not_vacuous prints them):
      bounded activation:  xyz 0.86   halved density 0.51   child scaling 0.39
      exp activation:      xyz 0.43   halved density 0.51   child scaling 0.63
* the comparator fails for each of twelve ways a kernel can be subtly wrong (densify_ref.MUTATIONS).
"""
import os

import numpy as np
import pytest
import torch

from tests import densify_ref as R
from tests import mini_trainer as T

GOLD = os.path.join(os.path.dirname(__file__), "golden", "train")
BOUND = (0.001, 1.0)


def _scene(P, scale_bound, prune_only=False):
    return R.edge_case(P, scale_bound, seed=P, prune_only=prune_only)


def test_float32_restatement_and_the_planted_rows_on_every_scene():
    for k, P in enumerate((1, 255, 256, 257, 4095, 4096, 4097, 8193)):   # the GPU test's scenes: edge_case's assertions hold
        for sb in (BOUND, None):
            inp, planted = R.edge_case(P, sb, seed=P, moments=k % 2 == 1)
            assert (len(planted) > 0) == (P >= 128)
            R.check(R.restate32(inp), inp, R.statement(inp))
    for P in (257, 4097):
        inp, planted = _scene(P, BOUND, prune_only=True)
        ref = R.statement(inp)
        R.check(R.restate32(inp), inp, ref)
        assert ref["counts"][1:] == (0, 0, 0) and not ref["stats_reset"]


@pytest.mark.parametrize("case", ["A", "B", "C"])
def test_statement_against_the_reference_fixtures(case):
    g = np.load(os.path.join(GOLD, "densify_%s.npz" % case))
    cfg = g["cfg"]   # max_grad, min_density, max_screen_size (0 = None), max_scale (0 = None), max_num_gaussians, scale_thr
    P = g["in.xyz"].shape[0]
    inp = R.make_inputs({n: g["in." + n] for n in R.NAMES}, {n: (g["in.%s.m" % n], g["in.%s.v" % n]) for n in R.NAMES},
                        g["in.max_radii2D"], g["in.grad_accum"], g["in.denom"], g["normals"], cfg[0], cfg[5], cfg[1], g["bbox"],
                        tuple(g["scale_bound"]), P < cfg[4], cfg[2], cfg[3])
    got = R.result_of({n: g["out." + n] for n in R.NAMES}, {n: (g["out.%s.m" % n], g["out.%s.v" % n]) for n in R.NAMES},
                      g["out.max_radii2D"], g["out.grad_accum"], g["out.denom"], None)
    ref = R.statement(inp)
    assert sum(ref["counts"]) == g["out.xyz"].shape[0] != P
    R.check(got, inp, ref)


def _torch_statement(inp):
    """mini_trainer.Model.densify_and_prune on the oracle backend (CPU), as tests/test_train_golden_cpu.py runs it."""
    lo, hi = (float(v) for v in inp["scale_bound"])
    opt = T.Opt(iterations=30000, densify_grad_threshold=float(inp["grad_thr"]), density_min_threshold=float(inp["density_min"]),
                max_screen_size=float(inp["max_screen"]) or None, max_scale=(float(inp["max_scale"]) / 2.0) or None,
                max_num_gaussians=10 ** 9 if inp["do_densify"] else 1, densify_scale_threshold=float(inp["scale_thr"]) / 2.0,
                scale_min=lo / 2.0, scale_max=hi / 2.0)            # the trainer multiplies by volume_to_world = 2: exact
    t = torch.from_numpy
    raw = {n: t(inp[n]) for n in R.NAMES}
    moments = {n: tuple(t(x) for x in inp["moments"][n]) for n in R.NAMES}
    m = T.Model.from_tensors(opt, T.Backend("oracle"), raw, moments, {n: 1.0 for n in R.NAMES}, t(inp["max_radii2D"]),
                             t(inp["grad_accum"])[:, None], t(inp["denom"])[:, None])
    m.densify_and_prune(t(inp["bbox"]), normals_full=t(inp["normals"]))
    st = {g["name"]: m.optimizer.state[g["params"][0]] for g in m.optimizer.param_groups}
    return R.result_of({n: m.p[n].detach().numpy() for n in R.NAMES},
                       {n: (st[n]["exp_avg"].numpy(), st[n]["exp_avg_sq"].numpy()) for n in R.NAMES},
                       m.max_radii2D.numpy(), m.grad_accum.numpy(), m.denom.numpy(), None)


@pytest.mark.parametrize("P", [257, 4097])
def test_statement_against_the_torch_statement_on_the_edge_scene(P):
    inp, planted = _scene(P, BOUND)
    assert len(planted) > 30
    R.check(_torch_statement(inp), inp, R.statement(inp))          # layout exact, every planted row included
    inp, planted = _scene(P, BOUND, prune_only=True)
    R.check(_torch_statement(inp), inp, R.statement(inp))


def test_the_bound_is_honest_and_not_vacuous():
    for sb in (BOUND, None):
        ratios = {}
        for P in (257, 4097):
            inp, _planted = _scene(P, sb)
            R.check(R.restate32(inp), inp, R.statement(inp), ratios)
        print("scale_bound %s: worst error / bound %s" % (sb, {k: round(v, 3) for k, v in ratios.items()}))
        assert set(ratios) == {"xyz", "density", "scaling"}, ratios          # rotations are copies
        assert all(0.05 <= v <= 1.0 for v in ratios.values()), ratios


@pytest.mark.parametrize("mutation", R.MUTATIONS)
def test_the_comparator_catches(mutation):
    inp, _planted = _scene(257, BOUND, prune_only=mutation == "density_le")   # the density threshold is planted in that scene
    ref = R.statement(inp)
    R.check(R.restate32(inp), inp, ref)
    with pytest.raises(AssertionError):
        R.check(R.restate32(inp, mutation), inp, ref)
    if mutation in ("scale_lt", "divide_by_1_5", "transposed_rotation", "child_density_unhalved"):   # and under exp scales
        inp, _planted = _scene(257, None)
        with pytest.raises(AssertionError):
            R.check(R.restate32(inp, mutation), inp, R.statement(inp))


def test_statistics_statement_bounds_the_float32_accumulation():
    for P in (1, 255, 256, 257):
        radii, g2d, mr, ga, dn = R.stats_case(P, seed=P)
        vis, mr_ref, acc, dn_ref = R.stats_statement(radii, g2d, mr, ga, dn)
        with np.errstate(all="ignore"):
            got = np.where(vis, ga + np.sqrt(g2d[:, 0] * g2d[:, 0] + g2d[:, 1] * g2d[:, 1]), ga)
        R.check_stats((mr_ref, got, dn_ref), (radii, g2d, mr, ga, dn))
        if P >= 255:
            assert np.isnan(acc.v).sum() == 1 and np.isposinf(acc.v).sum() >= 1 and (~vis).sum() > 10
