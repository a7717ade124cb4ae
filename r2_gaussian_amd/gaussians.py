"""GaussianModel on the MI355X kernels (r2_gaussian/gaussian/gaussian_model.py): raw parameters, Adam moments, per-group step
counts and learning-rate schedules, the densification statistics -- and one fused launch per training iteration
(``r2_gaussian_adam_step``, csrc/gaussian_step.hip) that chains the gradients through the activations, applies Adam over the
four groups and writes the next iteration's activated parameters.

Autograd sees only the ACTIVATED parameters, as leaf tensors (``activated()``): the rasterizer and voxelizer leave
dL/d(activation) in their ``.grad``, which is exactly what the step kernel takes.  xyz's activation is the identity, so its raw
tensor is the leaf.  ``capture()`` / ``restore()`` use the reference's 10-tuple with a ``torch.optim.Adam.state_dict()``, so
checkpoints move between this model and the reference's in both directions.
"""
import ctypes as C

import numpy as np
import torch
from torch import nn

from . import densify as D
from ._boundary import _F32, NAMES, WIDTHS, call, ptr_table, require_gpu

BETAS, ADAM_EPS = (0.9, 0.999), 1e-15      # gaussian_model.py:213 (torch.optim.Adam defaults, eps 1e-15)
EPS = 1e-5                                  # gaussian_model.py:34: keeps the initial scales inside the bound


def get_expon_lr_func(lr_init, lr_final, lr_delay_steps=0, lr_delay_mult=1.0, max_steps=1000000):
    """utils/gaussian_utils.py:13-46: lr_init at step 0, lr_final at max_steps, log-linear in between."""
    def helper(step):
        if step < 0 or (lr_init == 0.0 and lr_final == 0.0):
            return 0.0
        if lr_delay_steps > 0:
            delay_rate = lr_delay_mult + (1 - lr_delay_mult) * np.sin(0.5 * np.pi * np.clip(step / lr_delay_steps, 0, 1))
        else:
            delay_rate = 1.0
        t = np.clip(step / max_steps, 0, 1)
        return float(delay_rate * np.exp(np.log(lr_init) * (1 - t) + np.log(lr_final) * t))
    return helper


def _bound(scale_bound):
    """-> (lo, hi) as the C ABI takes them: (0, 0) = no bound (exp activation)."""
    if scale_bound is None:
        return 0.0, 0.0
    lo, hi = float(scale_bound[0]), float(scale_bound[1])
    assert lo < hi, "scale_min must be smaller than scale_max."
    return lo, hi


def activate(density, scaling, rotation, scale_bound=None):
    """-> (density_act [P,1], scaling_act [P,3], rotation_act [P,4]) of raw parameters: one launch (r2_gaussian_activate)."""
    require_gpu(density, "density")
    P = density.shape[0]
    dev = density.device
    lo, hi = _bound(scale_bound)
    ins = [t.detach().to(_F32).contiguous() for t in (density, scaling, rotation)]
    assert [tuple(t.shape) for t in ins] == [(P, 1), (P, 3), (P, 4)]
    outs = [torch.empty((P, WIDTHS[n]), dtype=_F32, device=dev) for n in NAMES[1:]]
    call("r2_gaussian_activate", dev, P, *ins, lo, hi, *outs)
    return tuple(outs)


class GaussianModel:
    """gaussian_model.py:GaussianModel with the optimizer replaced by the fused step.  Raw parameters: ``_xyz`` [P,3],
    ``_density`` [P,1], ``_scaling`` [P,3], ``_rotation`` [P,4]; Adam state: ``exp_avg`` / ``exp_avg_sq`` (dicts by group name)
    and ``steps`` (per group, as torch keeps one step count per parameter)."""

    def __init__(self, scale_bound=None, device="cuda"):
        self.scale_bound = None if scale_bound is None else np.asarray(scale_bound, dtype=np.float64)
        _bound(self.scale_bound)
        self.device = torch.device(device)
        self.spatial_lr_scale = 0.0
        self.schedules = None
        self.lr = {n: 0.0 for n in NAMES}
        self._set(*(torch.empty((0, WIDTHS[n]), dtype=_F32, device=self.device) for n in NAMES))

    # ------------------------------------------------------------------------------------------------ state
    def _set(self, xyz, density, scaling, rotation, moments=None, steps=None):
        """New raw parameters, Adam state (zero moments and step counts unless given) and activations; the densification
        statistics are the caller's to set."""
        raw = dict(zip(NAMES, (xyz, density, scaling, rotation)))
        self._raw = {n: raw[n].detach().to(device=self.device, dtype=_F32).contiguous().clone() for n in NAMES}
        P = self._raw["xyz"].shape[0]
        for n in NAMES:
            assert tuple(self._raw[n].shape) == (P, WIDTHS[n]), (n, tuple(self._raw[n].shape))
        self._raw["xyz"].requires_grad_(True)
        if moments is None:
            moments = {n: (torch.zeros_like(self._raw[n]), torch.zeros_like(self._raw[n])) for n in NAMES}
        self.exp_avg = {n: moments[n][0].to(device=self.device, dtype=_F32).contiguous() for n in NAMES}
        self.exp_avg_sq = {n: moments[n][1].to(device=self.device, dtype=_F32).contiguous() for n in NAMES}
        self.steps = dict(steps) if steps is not None else {n: 0 for n in NAMES}
        self._activate()

    def _activate(self):
        d, s, r = activate(self._raw["density"], self._raw["scaling"], self._raw["rotation"], self.scale_bound) if self.P else (
            torch.empty((0, WIDTHS[n]), dtype=_F32, device=self.device) for n in NAMES[1:])
        self._act = {"density": d.requires_grad_(True), "scaling": s.requires_grad_(True), "rotation": r.requires_grad_(True)}

    def _install(self, raw, moments, stats=None):
        """The rows a surgery returned: raw parameters and Adam moments (dicts by name) and the statistics (max_radii2D,
        grad_accum, denom; None: reset).  Step counts stay, the activations are refreshed."""
        self._raw = {n: raw[n] for n in NAMES}
        self._raw["xyz"].requires_grad_(True)
        self.exp_avg = {n: moments[n][0] for n in NAMES}
        self.exp_avg_sq = {n: moments[n][1] for n in NAMES}
        if stats is None:
            self._reset_stats()
        else:
            self.max_radii2D, self.xyz_gradient_accum, self.denom = stats[0], stats[1].reshape(-1, 1), stats[2].reshape(-1, 1)
        self._activate()

    def _raw_from_activated(self, density, scales):
        """-> (raw density, raw scales) through the inverse activations as gaussian_model.py:133-164 forms them: the inverse
        softplus, and the inverse scaling activation of the scales clamped EPS inside the bound.  On the inputs' devices."""
        density = torch.log(torch.exp(density) - 1)                                     # inverse_softplus
        if self.scale_bound is None:
            return density, torch.log(scales)
        lo, hi = self.scale_bound
        scales = torch.relu((torch.clamp(scales, lo + EPS, hi - EPS) - lo) / (hi - lo))
        return density, torch.log(scales / (1 - scales))                                # inverse_sigmoid

    def _reset_stats(self):
        self.max_radii2D = torch.zeros(self.P, dtype=_F32, device=self.device)
        self.xyz_gradient_accum = torch.zeros((self.P, 1), dtype=_F32, device=self.device)
        self.denom = torch.zeros((self.P, 1), dtype=_F32, device=self.device)

    @property
    def P(self):
        return self._raw["xyz"].shape[0]

    @property
    def _xyz(self):
        return self._raw["xyz"]

    @property
    def _density(self):
        return self._raw["density"]

    @property
    def _scaling(self):
        return self._raw["scaling"]

    @property
    def _rotation(self):
        return self._raw["rotation"]

    def activated(self):
        """-> (xyz, density, scaling, rotation): leaf tensors with requires_grad, what the drop-in rasterizer and voxelizer
        take.  The tensors are updated in place by ``step()``; gradients of several renders / queries accumulate in .grad."""
        return self._raw["xyz"], self._act["density"], self._act["scaling"], self._act["rotation"]

    @property
    def get_xyz(self):
        return self._raw["xyz"]

    @property
    def get_density(self):
        return self._act["density"]

    @property
    def get_scaling(self):
        return self._act["scaling"]

    @property
    def get_rotation(self):
        return self._act["rotation"]

    # ------------------------------------------------------------------------------------------------ set-up
    def create_from_pcd(self, xyz, density, spatial_lr_scale=1.0):
        """gaussian_model.py:133-164: raw density = inverse softplus, scales = the mean distance to the 3 nearest neighbours
        (clamped to >= 0.001 and into the scale bound) through the inverse scaling activation, identity rotations."""
        from ._C import distCUDA2
        self.spatial_lr_scale = spatial_lr_scale
        pts = torch.as_tensor(np.asarray(xyz), dtype=_F32).to(self.device).contiguous()
        dist = torch.sqrt(torch.clamp_min(distCUDA2(pts), 0.001 ** 2))
        dens, scales = self._raw_from_activated(torch.as_tensor(np.asarray(density), dtype=_F32).reshape(-1, 1), dist)
        dens, scales = dens.to(self.device), scales[..., None].repeat(1, 3)
        rots = torch.zeros((pts.shape[0], 4), dtype=_F32, device=self.device)
        rots[:, 0] = 1
        self._set(pts, dens, scales, rots)
        self._reset_stats()

    def training_setup(self, opt):
        """gaussian_model.py:188-240: the four groups' schedules (lr_init / lr_final * spatial_lr_scale, *_lr_max_steps)."""
        s = self.spatial_lr_scale
        self.schedules = {
            "xyz": get_expon_lr_func(opt.position_lr_init * s, opt.position_lr_final * s, max_steps=opt.position_lr_max_steps),
            "density": get_expon_lr_func(opt.density_lr_init * s, opt.density_lr_final * s, max_steps=opt.density_lr_max_steps),
            "scaling": get_expon_lr_func(opt.scaling_lr_init * s, opt.scaling_lr_final * s, max_steps=opt.scaling_lr_max_steps),
            "rotation": get_expon_lr_func(opt.rotation_lr_init * s, opt.rotation_lr_final * s,
                                          max_steps=opt.rotation_lr_max_steps),
        }
        self.lr = {"xyz": opt.position_lr_init * s, "density": opt.density_lr_init * s, "scaling": opt.scaling_lr_init * s,
                   "rotation": opt.rotation_lr_init * s}
        self._reset_stats()

    def update_learning_rate(self, iteration):
        for n in NAMES:
            self.lr[n] = self.schedules[n](iteration)

    # ------------------------------------------------------------------------------------------------ the step
    @torch.no_grad()
    def step(self, iteration=None, lr=None):
        """One optimizer step: the schedules at `iteration` (unless None), or the explicit per-group ``lr`` dict, then the
        fused kernel, then .grad = None.  Groups without .grad are skipped, as torch.optim.Adam skips them.  No host
        synchronisation."""
        if lr is not None:
            self.lr.update(lr)
        elif iteration is not None:
            self.update_learning_rate(iteration)
        leaves = self.activated()
        grads = []
        for n, t in zip(NAMES, leaves):
            g = t.grad
            if g is not None:
                assert g.dtype == _F32 and g.shape == t.shape, n
                g = g.contiguous()
                self.steps[n] += 1
            grads.append(g)
        if self.P:
            lrs = (C.c_double * 4)(*[float(self.lr[n]) for n in NAMES])
            bc1 = (C.c_double * 4)(*[1.0 - BETAS[0] ** self.steps[n] if g is not None else 1.0 for n, g in zip(NAMES, grads)])
            bc2 = (C.c_double * 4)(*[1.0 - BETAS[1] ** self.steps[n] if g is not None else 1.0 for n, g in zip(NAMES, grads)])
            lo, hi = _bound(self.scale_bound)
            a = self._act
            call("r2_gaussian_adam_step", self.device, self.P, ptr_table([self._raw[n] for n in NAMES]), ptr_table(grads),
                 ptr_table([self.exp_avg[n] for n in NAMES]), ptr_table([self.exp_avg_sq[n] for n in NAMES]), lrs, bc1, bc2, lo, hi,
                 a["density"], a["scaling"], a["rotation"])
        for t in leaves:
            t.grad = None

    # ------------------------------------------------------------------------------------------------ density control
    def add_densification_stats(self, radii, viewspace_grad, grad_scale=1.0):
        """train.py:151-154 in one launch: max_radii2D, xyz_gradient_accum, denom of the visible Gaussians.  radii [P] and
        viewspace_grad [P, 3] of one view, or [V, P] and [V, P, 3] of a batched render (the views in order, the gradient norms
        times grad_scale: densify.densification_stats_batch)."""
        if radii.dim() == 1 and grad_scale == 1.0:
            D.densification_stats(radii, viewspace_grad, self.max_radii2D, self.xyz_gradient_accum, self.denom)
            return
        if radii.dim() == 1:
            radii, viewspace_grad = radii[None], viewspace_grad[None]
        D.densification_stats_batch(radii, viewspace_grad, self.max_radii2D, self.xyz_gradient_accum, self.denom, grad_scale)

    @torch.no_grad()
    def densify_and_prune(self, max_grad, min_density, max_screen_size, max_scale, max_num_gaussians, densify_scale_threshold,
                          bbox, normals=None):
        """gaussian_model.py:503-550 through r2_gaussian_amd.densify; step counts are kept (cat_tensors_to_optimizer /
        _prune_optimizer keep the state's step), new rows get zero moments, then the parameters are re-activated.
        normals: [2,P,3] N(0,1) split samples (drawn here with torch.randn when None)."""
        if normals is None:
            normals = torch.randn((2, self.P, 3))
        new_p, new_m, mr, ga, dn, _cnt = D.densify_and_prune(
            dict(self._raw), {n: (self.exp_avg[n], self.exp_avg_sq[n]) for n in NAMES}, self.max_radii2D,
            self.xyz_gradient_accum, self.denom, normals, max_grad, densify_scale_threshold, min_density, bbox,
            self.scale_bound, do_densify=self.P < max_num_gaussians, max_screen_size=max_screen_size, max_scale=max_scale)
        self._install(new_p, new_m, (mr, ga, dn))

    @torch.no_grad()
    def merge(self, max_cost, k=8, rounds=12):
        """Merge neighbouring Gaussians that say the same thing (r2_gaussian_amd.merge, not in the reference): the edges of the
        k-NN graph whose Runnalls cost is <= max_cost are matched and every pair is replaced by its moment-matched Gaussian; with
        a scale bound no merged scale exceeds its upper end.  Survivors keep their raw parameters and Adam moments, bit for bit;
        a merged row gets raw parameters through the inverse activations, as create_from_pcd forms them, and zero moments, as
        the new rows of a densification do.  Step counts are kept, the densification statistics are reset, the activations
        refreshed.  -> number of pairs merged (one host read)."""
        from . import merge as MG
        if self.P < 2:
            return 0
        xyz, dens, scal, rot = (t.detach() for t in self.activated())
        hi = None if self.scale_bound is None else float(self.scale_bound[1])
        m_xyz, m_dens, m_scal, m_rot, src, info = MG.merge_gaussians(xyz, dens, scal, rot, max_cost, k=k, rounds=rounds,
                                                                     max_scale=hi)
        if info["pairs"] == 0:
            return 0
        keep = src[:, 0].long()
        merged = (src[:, 1] >= 0)[:, None]
        d, s = self._raw_from_activated(m_dens, m_scal)
        fresh = {"xyz": m_xyz, "density": d, "scaling": s, "rotation": m_rot}
        zero = torch.zeros((), dtype=_F32, device=self.device)
        raw = {n: torch.where(merged, fresh[n], self._raw[n].detach()[keep]) for n in NAMES}
        moments = {n: (torch.where(merged, zero, self.exp_avg[n][keep]), torch.where(merged, zero, self.exp_avg_sq[n][keep]))
                   for n in NAMES}
        self._install(raw, moments)
        return info["pairs"]

    @torch.no_grad()
    def add_noise(self, call, noise_lr=5e5, density=0.005, sharpness=0.5, seed=0):
        """Covariance-shaped Langevin noise on the positions of Gaussians whose density has faded (r2_gaussian_amd.mcmc, not in the
        reference): xyz += lr_xyz * noise_lr * gate * R S^2 R^T eps with the current xyz learning rate, gate = 1 / (1 + exp(
        sharpness (rho / density - 1))), eps from (seed, call, row): the trainer passes the iteration as `call`, so a resumed run
        draws what the uninterrupted one would.  In place on the raw xyz, from the activations as they stand (``_act`` after a
        step); moments and step counts are untouched.  The defaults are the original method's and untuned for CT.  No host read."""
        from . import mcmc as MC
        if self.P:
            a = self._act
            MC.position_noise(self._raw["xyz"], a["density"], a["scaling"], a["rotation"], float(self.lr["xyz"]) * float(noise_lr),
                              density_threshold=density, sharpness=sharpness, seed=seed, call=call)

    @torch.no_grad()
    def relocate(self, call, dead_density, cap_max, growth=0.05, spread=0.0, seed=0):
        """Keep a fixed budget (r2_gaussian_amd.mcmc.relocate, not in the reference): every Gaussian whose density is not above
        dead_density (or that holds a non-finite parameter) moves onto a live one drawn in proportion to its density, and
        n_new = max(0, min(cap_max, ceil((1 + growth) P)) - P) rows are appended the same way; a Gaussian drawn n times and its n
        copies share its density, so with spread = 0 the field is unchanged.  Moved, appended and drawn rows get zero Adam
        moments and statistics, every other row keeps its bits; step counts are kept, the activations refreshed.  -> n_new.
        No host read."""
        from . import mcmc as MC
        P = self.P
        if P == 0:
            return 0
        n_new = max(0, min(int(cap_max), int(np.ceil((1.0 + float(growth)) * P))) - P)
        a = self._act
        new_p, new_m, st, _info = MC.relocate(
            {n: self._raw[n].detach() for n in NAMES}, {n: (self.exp_avg[n], self.exp_avg_sq[n]) for n in NAMES},
            (self.max_radii2D, self.xyz_gradient_accum, self.denom), dead_density, n_new=n_new, spread=spread, seed=seed,
            call=call, activated=(a["density"].detach(), a["scaling"].detach(), a["rotation"].detach()))
        self._install(new_p, new_m, st)
        return n_new

    # ------------------------------------------------------------------------------------------------ files
    def save_ply(self, path):
        """point_cloud.pickle of RAW parameters (gaussian_model.py:263-286)."""
        from . import model_io
        model_io.save_point_cloud(path, self._raw["xyz"], self._raw["density"], self._raw["scaling"], self._raw["rotation"],
                                  self.scale_bound)

    def load_ply(self, path):
        from . import model_io
        d = model_io.load_point_cloud(path, device=self.device)
        if d.get("scale_bound") is not None:
            self.scale_bound = np.asarray(d["scale_bound"], dtype=np.float64)
        self._set(d["xyz"], d["density"], d["scaling"], d["rotation"])
        self._reset_stats()

    def _torch_adam(self):
        """A torch.optim.Adam laid out like the reference's (gaussian_model.py:192-215) over Parameters that share this model's
        storage: the one place where the state_dict format is produced and read."""
        params = {n: nn.Parameter(self._raw[n].detach()) for n in NAMES}
        opt = torch.optim.Adam([{"params": [params[n]], "lr": self.lr[n], "name": n} for n in NAMES], lr=0.0, eps=ADAM_EPS)
        return opt, params

    def optimizer_state(self):
        """-> torch.optim.Adam.state_dict() of the reference's optimizer holding this model's state (copies)."""
        opt, params = self._torch_adam()
        for n in NAMES:
            if self.steps[n] > 0:
                opt.state[params[n]] = {"step": torch.tensor(float(self.steps[n])), "exp_avg": self.exp_avg[n].clone(),
                                        "exp_avg_sq": self.exp_avg_sq[n].clone()}
        return opt.state_dict()

    def capture(self):
        """The reference's 10-tuple (gaussian_model.py:79-91): raw parameters as nn.Parameter copies, statistics, the Adam
        state_dict, spatial_lr_scale, scale_bound."""
        p = {n: nn.Parameter(self._raw[n].detach().clone()) for n in NAMES}
        return (p["xyz"], p["scaling"], p["rotation"], p["density"], self.max_radii2D.clone(), self.xyz_gradient_accum.clone(),
                self.denom.clone(), self.optimizer_state(), self.spatial_lr_scale, self.scale_bound)

    def restore(self, model_args, training_args=None):
        """gaussian_model.py:93-110: the 10-tuple of capture() (this model's or the reference's)."""
        (xyz, scaling, rotation, density, max_radii2D, grad_accum, denom, opt_dict, self.spatial_lr_scale,
         scale_bound) = model_args
        self.scale_bound = None if scale_bound is None else np.asarray(scale_bound, dtype=np.float64)
        self._set(xyz, density, scaling, rotation)
        if training_args is not None:
            self.training_setup(training_args)
        opt, params = self._torch_adam()
        opt.load_state_dict(opt_dict)      # torch's own checks (four groups of one parameter); casts to the parameters' device
        for g in opt.param_groups:
            self.lr[g["name"]] = g["lr"]
        for n in NAMES:
            st = opt.state.get(params[n])
            if st is not None and "exp_avg" in st:
                self.exp_avg[n] = st["exp_avg"].to(device=self.device, dtype=_F32).contiguous()
                self.exp_avg_sq[n] = st["exp_avg_sq"].to(device=self.device, dtype=_F32).contiguous()
                self.steps[n] = int(round(float(st["step"])))
        self.max_radii2D = max_radii2D.to(device=self.device, dtype=_F32).reshape(-1).contiguous()
        self.xyz_gradient_accum = grad_accum.to(device=self.device, dtype=_F32).reshape(-1, 1).contiguous()
        self.denom = denom.to(device=self.device, dtype=_F32).reshape(-1, 1).contiguous()


__all__ = ["GaussianModel", "activate", "get_expon_lr_func", "NAMES"]
