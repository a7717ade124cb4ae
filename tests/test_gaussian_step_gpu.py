"""GPU: the fused model step (r2_gaussian_adam_step) and activation (r2_gaussian_activate) of r2_gaussian_amd.gaussians against
the float64 restatement (tests/gaussian_step_ref.py) and against torch (autograd + torch.optim.Adam) on the device, 20
consecutive steps with a changing learning rate, edge rows and a group without gradient; plus host synchronisation, density
control, and the checkpoint format.

Every step is checked from the same float32 state (the restatement and torch take the kernel's previous output), so errors
do not compound.  Tolerances: parameters within 2 ulp + 1e-6 lr; activations within 2 ulp; exp_avg within 4 ulp of the
largest term of its update (b1 m + (1 - b1) g can cancel to far below its terms) and exp_avg_sq within 4 ulp, each plus the
rounding of the activation chain that produced g: 2 ulp of (1 - b1) |g| and 4 ulp of (1 - b2) g^2.  For the rotation, whose
gradient g/|q| - q^(q^.g)/|q| can itself cancel, |g| is replaced by |g|_1 / |q| (and 8 ulp of (1 - b2) of its square)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import gaussian_step_ref as R
from tests.test_gaussian_step_cpu import edge_params, grads_at, lr_at

pytestmark = pytest.mark.gpu
NAMES = R.NAMES
DEV = "cuda:0"
BOUND = (0.001, 1.0)


def _ulp(x):
    return torch.from_numpy(np.spacing(np.abs(x.detach().cpu().numpy().astype(np.float32)))).double()


def _check(name, got, ref, tol):
    err = (got.detach().double().cpu() - ref.detach().double().cpu()).abs()
    bad = err > tol
    assert not bad.any(), "%s: %d values out of tolerance, worst err %.3e (tol there %.3e)" % (
        name, int(bad.sum()), float(err[bad].max()), float(tol[bad][err[bad].argmax()]))


def _model(raw32, scale_bound):
    from r2_gaussian_amd.gaussians import GaussianModel
    m = GaussianModel(scale_bound, device=DEV)
    m._set(*(raw32[n] for n in NAMES))
    m._reset_stats()
    return m


def _state(model):
    return ({n: model._raw[n].detach().clone() for n in NAMES}, {n: model.exp_avg[n].clone() for n in NAMES},
            {n: model.exp_avg_sq[n].clone() for n in NAMES}, dict(model.steps))


def _check_step(t, prev, model, G, lr, scale_bound, ref_p, ref_m, ref_v, what):
    """model: after the step from `prev`; ref_*: float64 (or float32) results from the same state."""
    p0, m0, v0, _s = prev
    for n in NAMES:
        if G[n] is None:
            assert torch.equal(model._raw[n].detach(), p0[n]) and torch.equal(model.exp_avg[n], m0[n]), (t, n)
            continue
        _check("%s step %d %s param" % (what, t, n), model._raw[n], ref_p[n],
               2 * _ulp(ref_p[n]) + 1e-6 * lr[n])
        g = R.chain({k: p0[k].double() for k in NAMES}, {k: (G[k].double() if G[k] is not None else None) for k in NAMES},
                    scale_bound, torch.float32)[n]
        gs = g.abs()
        if n == "rotation":   # the projection g/d - q^(q^.g)/d cancels: its rounding is relative to |g|/d, not to the result
            q = p0[n].double()
            gs = torch.maximum(gs, G[n].double().abs().sum(1, keepdim=True) / q.norm(dim=1, keepdim=True).clamp_min(1e-12))
        term = torch.maximum((R.BETA1 * m0[n].double()).abs(), (1 - R.BETA1) * gs)
        _check("%s step %d %s exp_avg" % (what, t, n), model.exp_avg[n], ref_m[n],
               4 * _ulp(term) + 2 * _ulp((1 - R.BETA1) * gs))
        _check("%s step %d %s exp_avg_sq" % (what, t, n), model.exp_avg_sq[n], ref_v[n],
               4 * _ulp(ref_v[n]) + (8 if n == "rotation" else 4) * _ulp((1 - R.BETA2) * gs * gs))


def _rows(P, scale_bound):
    raw = edge_params(P, scale_bound, seed=P)
    return {n: raw[n].float().to(DEV) for n in NAMES}


@pytest.mark.parametrize("scale_bound", [BOUND, None], ids=["bounded", "exp"])
@pytest.mark.parametrize("P", [1, 63, 64, 65, 300_000])
def test_step_matches_float64_restatement(P, scale_bound):
    model = _model(_rows(P, scale_bound), scale_bound)
    for t in range(1, 21):
        G = grads_at(t, P, zero_rows=min(3, P // 8))
        G = {n: (None if G[n] is None else G[n].float().to(DEV)) for n in NAMES}
        lr = lr_at(t)
        prev = _state(model)
        for n, leaf in zip(NAMES, model.activated()):
            leaf.grad = None if G[n] is None else G[n].clone()
        model.step(lr=lr)
        steps = model.steps
        assert all(steps[n] == prev[3][n] + (G[n] is not None) for n in NAMES)
        d = lambda dct: {n: dct[n].double() for n in NAMES}   # noqa: E731
        rp, rm, rv, ra = R.step(d(prev[0]), {n: None if G[n] is None else G[n].double() for n in NAMES}, d(prev[1]), d(prev[2]),
                                lr, steps, scale_bound, saved=torch.float32)
        _check_step(t, prev, model, G, lr, scale_bound, rp, rm, rv, "ref")
        # the next activations the step wrote, against the restatement of the kernel's own new parameters
        act = R.activate({n: model._raw[n].detach().double() for n in NAMES}, scale_bound, saved=torch.float32)
        _, a_d, a_s, a_r = model.activated()
        for n, got in (("density", a_d), ("scaling", a_s), ("rotation", a_r)):
            _check("step %d activated %s" % (t, n), got, act[n], 2 * _ulp(act[n]))
        assert all(leaf.grad is None for leaf in model.activated())


def _torch_act(leaves, scale_bound):
    sc = (torch.sigmoid(leaves["scaling"]) * (scale_bound[1] - scale_bound[0]) + scale_bound[0]) if scale_bound is not None \
        else torch.exp(leaves["scaling"])
    return {"xyz": leaves["xyz"], "density": F.softplus(leaves["density"]), "scaling": sc,
            "rotation": F.normalize(leaves["rotation"])}


@pytest.mark.parametrize("scale_bound", [BOUND, None], ids=["bounded", "exp"])
@pytest.mark.parametrize("P", [65, 300_000])
def test_step_matches_torch_adam_on_device(P, scale_bound):
    model = _model(_rows(P, scale_bound), scale_bound)
    for t in range(1, 21):
        G = grads_at(t, P)
        G = {n: (None if G[n] is None else G[n].float().to(DEV)) for n in NAMES}
        lr = lr_at(t)
        prev = _state(model)
        # torch from the same float32 state
        leaves = {n: prev[0][n].clone().requires_grad_(True) for n in NAMES}
        opt = torch.optim.Adam([{"params": [leaves[n]], "lr": lr[n], "name": n} for n in NAMES], lr=0.0, eps=1e-15)
        for n in NAMES:
            if prev[3][n] > 0:
                opt.state[leaves[n]] = {"step": torch.tensor(float(prev[3][n])), "exp_avg": prev[1][n].clone(),
                                        "exp_avg_sq": prev[2][n].clone()}
        act = _torch_act(leaves, scale_bound)
        sum((act[n] * G[n]).sum() for n in NAMES if G[n] is not None).backward()
        opt.step()
        for n, leaf in zip(NAMES, model.activated()):
            leaf.grad = None if G[n] is None else G[n].clone()
        model.step(lr=lr)
        tp = {n: leaves[n].detach() for n in NAMES}
        tm = {n: opt.state[leaves[n]]["exp_avg"] if leaves[n] in opt.state else prev[1][n] for n in NAMES}
        tv = {n: opt.state[leaves[n]]["exp_avg_sq"] if leaves[n] in opt.state else prev[2][n] for n in NAMES}
        _check_step(t, prev, model, G, lr, scale_bound, tp, tm, tv, "torch")


@pytest.mark.parametrize("scale_bound", [BOUND, None], ids=["bounded", "exp"])
def test_activation_matches_torch(scale_bound):
    from r2_gaussian_amd.gaussians import activate
    raw = _rows(300_000, scale_bound)
    d, s, r = activate(raw["density"], raw["scaling"], raw["rotation"], scale_bound)
    ref = _torch_act(raw, scale_bound)
    for n, got in (("density", d), ("scaling", s), ("rotation", r)):
        _check("activated " + n, got, ref[n], 2 * _ulp(ref[n]))


def test_invalid_arguments_are_refused():
    from r2_gaussian_amd import _lib
    from r2_gaussian_amd.gaussians import activate
    raw = _rows(64, BOUND)
    with pytest.raises(AssertionError):
        activate(raw["density"], raw["scaling"], raw["rotation"], (1.0, 0.5))
    L = _lib.lib()
    out = torch.empty(64, 4, device=DEV)
    assert L.r2_gaussian_activate(64, raw["density"].data_ptr(), raw["scaling"].data_ptr(), raw["rotation"].data_ptr(), 1.0, 0.5,
                                  out.data_ptr(), out.data_ptr(), out.data_ptr(), None) == _lib.R2_ERR_INVALID
    assert L.r2_gaussian_activate(-1, None, None, None, 0.0, 0.0, None, None, None, None) == _lib.R2_ERR_INVALID
    assert L.r2_gaussian_activate(64, None, None, None, 0.0, 0.0, None, None, None, None) == _lib.R2_ERR_INVALID
    assert L.r2_gaussian_adam_step(64, None, None, None, None, None, None, None, 0.0, 0.0, None, None, None,
                                   None) == _lib.R2_ERR_INVALID


def test_step_makes_no_host_synchronisation():
    model = _model(_rows(300_000, BOUND), BOUND)
    for leaf in model.activated():
        leaf.grad = torch.randn_like(leaf)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        model.step(lr=lr_at(1))
        model.step(lr=lr_at(2))      # groups without .grad (all of them, after the first step)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    assert model.steps == {"xyz": 1, "density": 1, "scaling": 1, "rotation": 1}


def _trained_model(P=5000, steps=3):
    model = _model(_rows(P, BOUND), BOUND)
    g = torch.Generator(device=DEV).manual_seed(3)
    for t in range(1, steps + 1):
        for leaf in model.activated():
            leaf.grad = torch.randn(leaf.shape, generator=g, device=DEV)
        model.step(lr=lr_at(t))
    model.max_radii2D = torch.rand(P, generator=g, device=DEV) * 10
    model.xyz_gradient_accum = torch.rand((P, 1), generator=g, device=DEV) * 2e-4
    model.denom = torch.randint(0, 4, (P, 1), generator=g, device=DEV).float()
    return model


def test_densify_and_prune_matches_torch_adam_path():
    from r2_gaussian_amd import densify as D
    model = _trained_model()
    P = model.P
    params = {n: torch.nn.Parameter(model._raw[n].detach().clone()) for n in NAMES}
    opt = torch.optim.Adam([{"params": [params[n]], "lr": 0.0, "name": n} for n in NAMES], lr=0.0, eps=1e-15)
    for n in NAMES:
        opt.state[params[n]] = {"step": torch.tensor(float(model.steps[n])), "exp_avg": model.exp_avg[n].clone(),
                                "exp_avg_sq": model.exp_avg_sq[n].clone()}
    normals = torch.randn((2, P, 3), generator=torch.Generator().manual_seed(5))
    bbox = torch.tensor([[-2.0, -2.0, -2.0], [2.0, 2.0, 2.0]])
    args = (5e-5, 1e-5, None, None, 500_000, 0.2, bbox)
    new_p, mr, ga, dn = D.densify_and_prune_optimizer(opt, model.max_radii2D.clone(), model.xyz_gradient_accum.clone(),
                                                      model.denom.clone(), normals, args[0], args[5], args[1], bbox,
                                                      BOUND, do_densify=True)
    steps = dict(model.steps)
    model.densify_and_prune(*args, normals=normals)
    assert model.P == new_p["xyz"].shape[0] and model.P != P
    for n in NAMES:
        assert torch.equal(model._raw[n].detach(), new_p[n].detach()), n
        st = opt.state[new_p[n]]
        assert torch.equal(model.exp_avg[n], st["exp_avg"]) and torch.equal(model.exp_avg_sq[n], st["exp_avg_sq"]), n
    assert model.steps == steps
    assert torch.equal(model.max_radii2D, mr) and torch.equal(model.xyz_gradient_accum, ga) and torch.equal(model.denom, dn)
    from r2_gaussian_amd.gaussians import activate
    for got, ref in zip(model.activated()[1:], activate(model._density, model._scaling, model._rotation, BOUND)):
        assert torch.equal(got.detach(), ref) and got.requires_grad and got.is_leaf


def test_capture_loads_into_torch_adam_and_restores(tmp_path):
    from r2_gaussian_amd import model_io
    from r2_gaussian_amd.gaussians import GaussianModel
    model = _trained_model()
    cap = model.capture()
    assert len(cap) == len(model_io.CAPTURE_FIELDS)
    model_io.save_checkpoint(str(tmp_path / "chkpnt3.pth"), cap, 3)
    loaded, it = model_io.load_checkpoint(str(tmp_path / "chkpnt3.pth"))
    assert it == 3
    # the reference's training_setup + restore: Adam over (xyz, density, scaling, rotation), load_state_dict
    params = [loaded["xyz"], loaded["density"], loaded["scaling"], loaded["rotation"]]
    opt = torch.optim.Adam([{"params": [p], "lr": 0.0, "name": n} for n, p in zip(NAMES, params)], lr=0.0, eps=1e-15)
    opt.load_state_dict(loaded["optimizer_state"])
    for n, p in zip(NAMES, params):
        st = opt.state[p]
        assert int(st["step"]) == 3
        assert torch.equal(st["exp_avg"], model.exp_avg[n]) and torch.equal(st["exp_avg_sq"], model.exp_avg_sq[n])
        assert torch.equal(p.detach(), model._raw[n].detach())
    # a model restored from the capture steps identically
    other = GaussianModel(None, device=DEV)
    other.restore(cap)
    assert other.steps == model.steps and np.array_equal(other.scale_bound, model.scale_bound)
    g = torch.Generator(device=DEV).manual_seed(9)
    grads = [torch.randn(t.shape, generator=g, device=DEV) for t in model.activated()]
    for m in (model, other):
        for leaf, gr in zip(m.activated(), grads):
            leaf.grad = gr.clone()
        m.step(lr=lr_at(4))
    for n in NAMES:
        assert torch.equal(model._raw[n], other._raw[n]) and torch.equal(model.exp_avg_sq[n], other.exp_avg_sq[n]), n
    for a, b in zip(model.activated(), other.activated()):
        assert torch.equal(a.detach(), b.detach())
