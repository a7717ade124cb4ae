"""csrc/densify_ops.hip (r2_densify_stats, r2_densify_classify, r2_densify_emit) against the float64 statement of
tests/densify_ref.py, at the edges: rows planted exactly on every threshold with their neighbours on the wrong side, 0 / 0 and
x / 0 gradients, a NaN coordinate, a zero quaternion, children shrunk under the scale bound, both scaling activations, P on both
sides of a workgroup (256) and of a scan tile (4096, binning.hip SC_TILE) with survivors of every kind across them.  No tolerance
here is a constant: every computed value has the bound the statement derives for it, everything else is bit equality
(tests/test_densify_ref_cpu.py shows on the CPU that the bound is honest, that the comparator catches a kernel subtly wrong, and
that the statement agrees with the reference's own code on every planted row)."""
import ctypes as C

import numpy as np
import pytest
import torch

from r2_gaussian_amd import _lib
from r2_gaussian_amd._boundary import ptr_table
from tests import densify_ref as R

pytestmark = pytest.mark.gpu
BOUND = (0.001, 1.0)
SHAPES = (1, 255, 256, 257, 4095, 4096, 4097, 8193)
_scenes = {}


def _scene(P, scale_bound, prune_only=False, moments=True):
    """edge_case once per shape; the tests share it and leave it unchanged."""
    key = (P, scale_bound, prune_only, moments)
    if key not in _scenes:
        inp, planted = R.edge_case(P, scale_bound, seed=P, prune_only=prune_only, moments=moments)
        _scenes[key] = (inp, planted, R.statement(inp))
    return _scenes[key]


def _args(inp, gpu):
    """The arguments of densify.densify_and_prune from a scene: fresh device tensors."""
    t = lambda a: torch.from_numpy(a).to(gpu)                     # noqa: E731
    params = {n: t(inp[n]) for n in R.NAMES}
    moments = None if inp["moments"] is None else {n: tuple(t(x) for x in inp["moments"][n]) for n in R.NAMES}
    sb = None if inp["scale_bound"] is None else tuple(float(v) for v in inp["scale_bound"])
    return [params, moments, t(inp["max_radii2D"]), t(inp["grad_accum"]), t(inp["denom"]), t(inp["normals"]), float(inp["grad_thr"]),
            float(inp["scale_thr"]), float(inp["density_min"]), torch.from_numpy(inp["bbox"])], dict(
                scale_bound=sb, do_densify=inp["do_densify"], max_screen_size=float(inp["max_screen"]), max_scale=float(inp["max_scale"]))


def _host(out):
    new_p, new_m, mr, ga, dn, cnt = out
    return R.result_of({n: new_p[n].cpu().numpy() for n in R.NAMES},
                       None if new_m is None else {n: tuple(x.cpu().numpy() for x in new_m[n]) for n in R.NAMES},
                       mr.cpu().numpy(), ga.cpu().numpy(), dn.cpu().numpy(), cnt)


def _same_bits(a, b):
    flat = lambda r: [r[n] for n in R.NAMES] + [r[k] for k in ("max_radii2D", "grad_accum", "denom")] + (   # noqa: E731
        [] if r["moments"] is None else [x for n in R.NAMES for x in r["moments"][n]])
    return a["counts"] == b["counts"] and all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(flat(a), flat(b)))


@pytest.mark.parametrize("scale_bound", [BOUND, None], ids=["bounded", "exp"])
@pytest.mark.parametrize("P", SHAPES)
def test_densify_matches_float64_at_the_edges(P, scale_bound, gpu):
    from r2_gaussian_amd import densify as D
    inp, planted, ref = _scene(P, scale_bound, moments=SHAPES.index(P) % 2 == 1)
    args, kw = _args(inp, gpu)
    before = _host((args[0], args[1], args[2], args[3], args[4], None))
    got = _host(D.densify_and_prune(*args, **kw))
    R.check(got, inp, ref)
    again = _host(D.densify_and_prune(*args, **kw))
    assert _same_bits(got, again)                                 # the same inputs, the same bits
    after = _host((args[0], args[1], args[2], args[3], args[4], None))
    assert _same_bits(before, after) and np.array_equal(args[5].cpu().numpy().view(np.uint32), inp["normals"].view(np.uint32))


@pytest.mark.parametrize("P", [257, 4097])
def test_prune_only_at_the_edges(P, gpu):
    from r2_gaussian_amd import densify as D
    inp, planted, ref = _scene(P, BOUND, prune_only=True)
    args, kw = _args(inp, gpu)
    got = _host(D.densify_and_prune(*args, **kw))
    R.check(got, inp, ref)                                        # the statistics carried over bit for bit, not zeroed
    hot = R.decide32(dict(inp, do_densify=True))
    assert (hot["clone"] | hot["split"]).sum() > P // 8           # hot rows exist ...
    assert got["counts"][1:] == (0, 0, 0) and got["grad_accum"].any() and got["denom"].any()   # ... and nothing is emitted for them
    kept = set(ref["src"].tolist())
    assert planted["density on"][0] in kept and planted["density below"][0] not in kept
    assert planted["hot, no densification"][0] in kept


def test_model_and_optimizer_paths_agree(gpu):
    """GaussianModel.densify_and_prune and densify_and_prune_optimizer on the exp activation across a scan tile equal the plain
    call bit for bit (tests/test_gaussian_step_gpu.py has the bounded activation at a small P)."""
    from r2_gaussian_amd import densify as D
    from r2_gaussian_amd.gaussians import GaussianModel
    inp, _planted, ref = _scene(4097, None)
    args, kw = _args(inp, gpu)
    plain = _host(D.densify_and_prune(*args, **kw))
    R.check(plain, inp, ref)
    params, moments, mr, ga, dn, normals, grad_thr, scale_thr, density_min, bbox = args
    # torch.optim.Adam with the reference's four groups
    leaves = {n: torch.nn.Parameter(params[n].clone()) for n in R.NAMES}
    opt = torch.optim.Adam([{"params": [leaves[n]], "lr": 0.0, "name": n} for n in R.NAMES], lr=0.0, eps=1e-15)
    for n in R.NAMES:
        opt.state[leaves[n]] = {"step": torch.tensor(3.0), "exp_avg": moments[n][0].clone(), "exp_avg_sq": moments[n][1].clone()}
    new_p, o_mr, o_ga, o_dn = D.densify_and_prune_optimizer(opt, mr.clone(), ga.clone()[:, None], dn.clone()[:, None], normals, grad_thr,
                                                            scale_thr, density_min, bbox, **kw)
    via_opt = R.result_of({n: new_p[n].detach().cpu().numpy() for n in R.NAMES},
                          {n: (opt.state[new_p[n]]["exp_avg"].cpu().numpy(), opt.state[new_p[n]]["exp_avg_sq"].cpu().numpy())
                           for n in R.NAMES}, o_mr.cpu().numpy(), o_ga.cpu().numpy(), o_dn.cpu().numpy(), plain["counts"])
    assert _same_bits(plain, via_opt) and all(float(opt.state[new_p[n]]["step"]) == 3.0 for n in R.NAMES)
    # the model with the fused step
    m = GaussianModel(None, device=gpu)
    m._set(*(params[n] for n in R.NAMES), moments={n: tuple(x.clone() for x in moments[n]) for n in R.NAMES},
           steps={n: 3 for n in R.NAMES})
    m.max_radii2D, m.xyz_gradient_accum, m.denom = mr.clone(), ga.clone()[:, None], dn.clone()[:, None]
    m.densify_and_prune(grad_thr, density_min, kw["max_screen_size"], kw["max_scale"], 10 ** 9, scale_thr, bbox, normals=normals)
    via_model = R.result_of({n: m._raw[n].detach().cpu().numpy() for n in R.NAMES},
                            {n: (m.exp_avg[n].cpu().numpy(), m.exp_avg_sq[n].cpu().numpy()) for n in R.NAMES},
                            m.max_radii2D.cpu().numpy(), m.xyz_gradient_accum.cpu().numpy(), m.denom.cpu().numpy(), plain["counts"])
    assert _same_bits(plain, via_model) and m.steps == {n: 3 for n in R.NAMES}


@pytest.mark.parametrize("P", [1, 255, 256, 257])
def test_stats_kernel_at_the_edges(P, gpu):
    from r2_gaussian_amd import densify as D
    case = R.stats_case(P, seed=P)
    radii, g2d, mr, ga, dn = (torch.from_numpy(a).to(gpu) for a in case)
    D.densification_stats(radii, g2d, mr, ga, dn)
    R.check_stats((mr.cpu().numpy(), ga.cpu().numpy(), dn.cpu().numpy()), case)
    assert np.array_equal(radii.cpu().numpy(), case[0]) and np.array_equal(g2d.cpu().numpy().view(np.uint32), case[1].view(np.uint32))


def test_validation_before_any_launch(gpu):
    L = _lib.lib()
    P, SENTINEL = 64, 7.0
    full = lambda *shape: torch.full(shape, SENTINEL, device=gpu)   # noqa: E731
    ins = {n: torch.rand(P, R.WIDTHS[n], device=gpu) for n in R.NAMES}
    m_in, v_in = ([torch.rand(P, R.WIDTHS[n], device=gpu) for n in R.NAMES] for _ in range(2))
    mr, ga, dn, normals = (torch.rand(s, device=gpu) for s in ((P,), (P,), (P,), (2, P, 3)))
    outs, m_out, v_out = ([full(2 * P, R.WIDTHS[n]) for n in R.NAMES] for _ in range(3))
    mr_o, ga_o, dn_o = full(2 * P), full(2 * P), full(2 * P)
    scratch = torch.full((int(L.r2_densify_scratch_bytes(P)),), 7, dtype=torch.uint8, device=gpu)
    box = (C.c_float * 6)(-1, -1, -1, 1, 1, 1)
    counts = (C.c_uint * 4)(7, 7, 7, 7)
    radii, g2d = torch.ones(P, dtype=torch.int32, device=gpu), torch.rand(P, 3, device=gpu)
    s_mr, s_ga, s_dn = full(P), full(P), full(P)
    ptr = lambda a: a.data_ptr() if isinstance(a, torch.Tensor) else a   # noqa: E731

    def invalid(name, args):
        rc = getattr(L, name)(*[ptr(a) for a in args], None)
        assert rc == _lib.R2_ERR_INVALID, (name, rc)
        assert name.encode() in L.r2_last_error(), (name, L.r2_last_error())

    def each_null(name, args, pointers):
        for k in pointers:
            invalid(name, args[:k] + [None] + args[k + 1:])

    cfg = [1e-4, 0.1, 1e-5, box, 0.001, 1.0, 1, 0.0, 0.0]
    stats = [P, radii, g2d, s_mr, s_ga, s_dn]
    each_null("r2_densify_stats", stats, range(1, 6))
    invalid("r2_densify_stats", [-1] + stats[1:])
    assert L.r2_densify_stats(0, None, None, None, None, None, None) == 0            # P == 0: nothing to do
    classify = [P] + [ins[n] for n in R.NAMES] + [mr, ga, dn, normals] + cfg + [scratch, counts]
    each_null("r2_densify_classify", classify, [1, 2, 3, 4, 5, 6, 7, 8, 12, 18, 19])
    for bad_P in (0, -1):
        invalid("r2_densify_classify", [bad_P] + classify[1:])
    tin, tout = ptr_table([ins[n] for n in R.NAMES]), ptr_table(outs)
    tm, tv, tmo, tvo = ptr_table(m_in), ptr_table(v_in), ptr_table(m_out), ptr_table(v_out)

    def emit(params=tin, m=None, v=None, params_out=tout, mo=None, vo=None):
        return [P, params, m, v, mr, ga, dn, normals] + cfg + [scratch, params_out, mo, vo, mr_o, ga_o, dn_o]

    each_null("r2_densify_emit", emit(), [1, 4, 5, 6, 7, 11, 17, 18, 21, 22, 23])
    for bad_P in (0, -1):
        invalid("r2_densify_emit", [bad_P] + emit()[1:])
    for k in range(4):                                            # a NULL inside a parameter table
        for key in ("params", "params_out"):
            tensors = [ins[n] for n in R.NAMES] if key == "params" else list(outs)
            tensors[k] = None
            invalid("r2_densify_emit", emit(**{key: ptr_table(tensors)}))
    invalid("r2_densify_emit", emit(m=tm, mo=tmo))                # exp_avg without exp_avg_sq
    invalid("r2_densify_emit", emit(v=tv, vo=tvo))
    invalid("r2_densify_emit", emit(m=tm, v=tv))                  # the input tables without their output tables
    invalid("r2_densify_emit", emit(m=tm, v=tv, mo=tmo))
    invalid("r2_densify_emit", emit(mo=tmo, vo=tvo))
    invalid("r2_densify_emit", emit(m=tm, v=tv, mo=tmo, vo=ptr_table([v_out[0], None, v_out[2], v_out[3]])))
    torch.cuda.synchronize()
    for t in outs + m_out + v_out + [mr_o, ga_o, dn_o, s_mr, s_ga, s_dn]:
        assert bool((t == SENTINEL).all())                        # nothing was launched into them
    assert bool((scratch == 7).all()) and list(counts) == [7, 7, 7, 7]
