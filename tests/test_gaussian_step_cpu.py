"""CPU: the float64 restatement of the fused model step (tests/gaussian_step_ref.py) equals torch in float64 -- the reference's
activations, autograd through them, and torch.optim.Adam(eps=1e-15) with four groups -- over 20 steps with a changing learning
rate, groups without a gradient, and the edge rows the GPU test uses."""
import pytest
import torch
import torch.nn.functional as F

from tests import gaussian_step_ref as R

NAMES = R.NAMES
WIDTHS = {"xyz": 3, "density": 1, "scaling": 3, "rotation": 4}


def edge_params(P, scale_bound, seed=0):
    """Raw parameters [P, w] in float64 with edge rows first: density > 20 and < -20, saturated sigmoid scales (with a bound),
    |q| from 1e-3 to 1e3."""
    g = torch.Generator().manual_seed(seed)
    raw = {"xyz": torch.randn(P, 3, generator=g, dtype=torch.float64),
           "density": torch.randn(P, 1, generator=g, dtype=torch.float64) * 3,
           "scaling": torch.randn(P, 3, generator=g, dtype=torch.float64) * (3 if scale_bound is not None else 1) - (
               0 if scale_bound is not None else 4),
           "rotation": torch.randn(P, 4, generator=g, dtype=torch.float64)}
    n = min(P, 8)
    edge_density = torch.tensor([25.0, 20.5, -21.0, -30.0, 20.0, -20.0, 0.0, 60.0], dtype=torch.float64)[:n]
    raw["density"][:n, 0] = edge_density
    if scale_bound is not None:
        raw["scaling"][:n] = torch.tensor([30.0, -30.0, 17.0], dtype=torch.float64)
    qn = torch.logspace(-3, 3, n, dtype=torch.float64)[:, None]
    raw["rotation"][:n] = raw["rotation"][:n] / raw["rotation"][:n].norm(dim=1, keepdim=True) * qn
    return raw


def grads_at(t, P, seed=1, zero_rows=3):
    g = torch.Generator().manual_seed(seed * 1000 + t)
    out = {n: torch.randn(P, WIDTHS[n], generator=g, dtype=torch.float64) * 10.0 ** (t % 3 - 1) for n in NAMES}
    for n in NAMES:
        out[n][-zero_rows:] = 0.0           # rows with a zero gradient
    if t % 5 == 2:
        out[NAMES[t % 4]] = None            # a group without .grad this step
    return out


def lr_at(t):
    return {"xyz": 2e-4 * 0.97 ** t, "density": 1e-2 * 0.9 ** t, "scaling": 5e-3 * (1 + 0.05 * t), "rotation": 1e-3 / t}


@pytest.mark.parametrize("scale_bound", [(0.001, 1.0), None], ids=["bounded", "exp"])
def test_restatement_equals_torch_float64(scale_bound):
    P = 40
    raw0 = edge_params(P, scale_bound)
    leaves = {n: raw0[n].clone().requires_grad_(True) for n in NAMES}
    opt = torch.optim.Adam([{"params": [leaves[n]], "lr": 0.0, "name": n} for n in NAMES], lr=0.0, eps=1e-15)
    lo_hi = scale_bound
    raw = {n: raw0[n].clone() for n in NAMES}
    m = {n: torch.zeros_like(raw[n]) for n in NAMES}
    v = {n: torch.zeros_like(raw[n]) for n in NAMES}
    steps = {n: 0 for n in NAMES}
    for t in range(1, 21):
        G = grads_at(t, P)
        lr = lr_at(t)
        # torch: activations, a loss whose gradient w.r.t. each activated tensor is G, autograd, Adam
        sc = (torch.sigmoid(leaves["scaling"]) * (lo_hi[1] - lo_hi[0]) + lo_hi[0]) if lo_hi is not None else torch.exp(
            leaves["scaling"])
        act = {"xyz": leaves["xyz"], "density": F.softplus(leaves["density"]), "scaling": sc,
               "rotation": F.normalize(leaves["rotation"])}
        loss = sum((act[n] * G[n]).sum() for n in NAMES if G[n] is not None)
        loss.backward()
        for gr in opt.param_groups:
            gr["lr"] = lr[gr["name"]]
        opt.step()
        opt.zero_grad(set_to_none=True)
        # the restatement
        for n in NAMES:
            if G[n] is not None:
                steps[n] += 1
        raw, m, v, a = R.step(raw, G, m, v, lr, steps, scale_bound)
        for n in NAMES:
            assert torch.allclose(raw[n], leaves[n].detach(), rtol=1e-12, atol=1e-15), (t, n)
            st = opt.state.get(leaves[n])
            if st is None:
                assert steps[n] == 0 and not m[n].any()
                continue
            assert int(st["step"]) == steps[n]
            assert torch.allclose(m[n], st["exp_avg"], rtol=1e-12, atol=1e-300), (t, n)
            assert torch.allclose(v[n], st["exp_avg_sq"], rtol=1e-12, atol=1e-300), (t, n)
        with torch.no_grad():
            sc = (torch.sigmoid(leaves["scaling"]) * (lo_hi[1] - lo_hi[0]) + lo_hi[0]) if lo_hi is not None else torch.exp(
                leaves["scaling"])
            ta = {"density": F.softplus(leaves["density"]), "scaling": sc, "rotation": F.normalize(leaves["rotation"])}
        for n in ta:
            assert torch.allclose(a[n], ta[n], rtol=1e-13, atol=0), (t, n)


def test_saturated_sigmoid_has_no_gradient_in_float32():
    """saved=float32: a sigmoid that rounds to exactly 1 (or 0) in float32 passes no gradient, as in a float32 torch model."""
    raw = {"xyz": torch.zeros(1, 3, dtype=torch.float64), "density": torch.zeros(1, 1, dtype=torch.float64),
           "scaling": torch.tensor([[30.0, -120.0, 0.0]], dtype=torch.float64),
           "rotation": torch.tensor([[1.0, 0, 0, 0]], dtype=torch.float64)}
    g = {"xyz": None, "density": None, "scaling": torch.ones(1, 3, dtype=torch.float64), "rotation": None}
    out32 = R.chain(raw, g, (0.001, 1.0), saved=torch.float32)["scaling"]
    out64 = R.chain(raw, g, (0.001, 1.0))["scaling"]
    assert out32[0, 0] == 0 and out32[0, 1] == 0 and out32[0, 2] > 0
    assert out64[0, 0] > 0
