"""Float64 restatement of the model step (csrc/gaussian_step.hip, r2_gaussian_amd.gaussians): the parameter activations of
gaussian_model.py:38-64, 112-126, their derivatives as torch's backward formulas compute them, and torch.optim.Adam's update in
its non-fused order (betas (0.9, 0.999), eps 1e-15; gaussian_model.py:188-215).  Test infrastructure.

All functions take and return float64 tensors (any device) in dicts keyed by group name (xyz, density, scaling, rotation).
``saved``: the dtype torch would hold the activations' saved OUTPUTS in (sigmoid and exp backward read their result, not their
input).  None (float64 throughout) is torch in float64; with torch.float32 those outputs are the ones a float32 model holds
(the sigmoid's is torch's own float32 sigmoid), so that a float32 sigmoid that saturates to exactly 1 has exactly zero
derivative here too.
"""
import torch

NAMES = ("xyz", "density", "scaling", "rotation")
BETA1, BETA2, EPS = 0.9, 0.999, 1e-15


def _round(t, saved):
    return t if saved is None else t.to(saved).double()


def sigmoid(x, saved=None):
    """torch.sigmoid in float64, or with `saved` the value torch computes in that dtype: its kernel evaluates
    1 / (1 + exp(-x)) with every step rounded, so in float32 the output is exactly 1 from x ~ 16.6 on, and the derivative
    (1 - y) y, which loses the low bits of y, is taken of that very y."""
    if saved is None:
        return torch.sigmoid(x)
    return torch.sigmoid(x.to(saved)).double()


def softplus(x):
    return torch.where(x > 20.0, x, torch.log1p(torch.exp(torch.clamp(x, max=20.0))))


def activate(raw, scale_bound=None, saved=None):
    """-> dict(density, scaling, rotation) activated (xyz's activation is the identity)."""
    x = raw["scaling"]
    if scale_bound is not None:
        lo, hi = float(scale_bound[0]), float(scale_bound[1])
        scaling = sigmoid(x, saved) * (hi - lo) + lo
    else:
        scaling = torch.exp(x)
    q = raw["rotation"]
    d = q.norm(dim=1, keepdim=True).clamp_min(1e-12)
    return {"density": softplus(raw["density"]), "scaling": scaling, "rotation": q / d}


def chain(raw, grads, scale_bound=None, saved=None):
    """dL/d(raw) from dL/d(activated) (None entries stay None)."""
    out = {"xyz": grads["xyz"]}
    g = grads["density"]
    if g is not None:
        x = raw["density"]
        z = torch.exp(torch.clamp(x, max=20.0))
        out["density"] = torch.where(x > 20.0, g, g * z / (z + 1.0))                  # softplus_backward
    else:
        out["density"] = None
    g = grads["scaling"]
    if g is not None:
        x = raw["scaling"]
        if scale_bound is not None:
            lo, hi = float(scale_bound[0]), float(scale_bound[1])
            y = sigmoid(x, saved)
            out["scaling"] = g * (hi - lo) * (1.0 - y) * y                            # mul, then sigmoid_backward
        else:
            out["scaling"] = g * _round(torch.exp(x), saved)
    else:
        out["scaling"] = None
    g = grads["rotation"]
    if g is not None:
        q = raw["rotation"]
        n = _round(q.norm(dim=1, keepdim=True), saved)
        d = n.clamp_min(1e-12)
        qh = q / d
        # (g - q^(q^.g)) / |q| for |q| >= 1e-12 (F.normalize's clamp passes no gradient below it)
        out["rotation"] = torch.where(n >= 1e-12, (g - qh * (qh * g).sum(1, keepdim=True)) / d, g / d)
    else:
        out["rotation"] = None
    return out


def adam(p, m, v, g, lr, step):
    """One torch.optim.Adam update of one tensor at step count `step` (after its increment) -> (p, m, v)."""
    m = m + (1 - BETA1) * (g - m)                         # lerp_(g, 1 - beta1)
    v = v * BETA2 + (1 - BETA2) * g * g
    bc1 = 1 - BETA1 ** step
    bc2 = 1 - BETA2 ** step
    denom = v.sqrt() / (bc2 ** 0.5) + EPS
    return p - (lr / bc1) * (m / denom), m, v


def step(raw, grads, exp_avg, exp_avg_sq, lr, steps, scale_bound=None, saved=None):
    """The fused step: chain rule, Adam per group (groups whose grad is None are left as they are; `steps` are the counts
    AFTER this step's increment), and the next activations.  -> (raw, exp_avg, exp_avg_sq, activated)."""
    graw = chain(raw, grads, scale_bound, saved)
    new_p, new_m, new_v = dict(raw), dict(exp_avg), dict(exp_avg_sq)
    for n in NAMES:
        if graw[n] is not None:
            new_p[n], new_m[n], new_v[n] = adam(raw[n], exp_avg[n], exp_avg_sq[n], graw[n], lr[n], steps[n])
    return new_p, new_m, new_v, activate(new_p, scale_bound, saved)
