"""R2-Gaussian training on the MI355X kernels: train.py:34-330 of the reference for a case in datagen's layout, on
``gaussians.GaussianModel`` (one fused HIP launch for the activations' backward, Adam and the next activations) and the
package's rasterizer, voxelizer, fused losses and fused density control.

    python -m r2_gaussian_amd.train -s <case> -m <output> [--iterations N] [--test_iterations ...] [...]

Flag names and defaults are the reference's (ModelParams, OptimizationParams, PipelineParams and train.py's own); an unknown
flag is an error.  ``training()`` is the loop itself: it takes views, projections, the ground truth, the geometry and the
initial points, so it runs as well on an in-memory case.  Outputs, in the reference's layout under the model path:
``point_cloud/iteration_N/{point_cloud.pickle, vol_gt.npy, vol_pred.npy}``, ``eval/iter_NNNNNN/{eval3d.yml,
eval2d_render_train.yml, eval2d_render_test.yml}``, ``ckpt/chkpnt{N}.pth``.  ``--eval_exact`` (not a flag of the reference; off
by default) adds ``eval2d_render_{train,test}_exact.yml``: the same 2D metrics on the exact projection of the model.
``--save_uncertainty LAMBDA`` (not a flag of the reference; off by default) adds ``fisher.npz`` and ``vol_std.npy`` to the last
``point_cloud/iteration_N``: the Fisher diagonal of the model over the training views and the standard deviation of the field
on the evaluation grid under the prior precision LAMBDA (uncertainty.py).

``--views_per_step W`` (not a flag of the reference; default 1 = its loop): one optimiser step on W views -- one batched
render, one batched loss node (the mean over the views), one backward, one batched statistics launch, one model step.
Iterations, the densification window and the learning-rate horizons then count optimiser steps, and the learning rates are
NOT rescaled: DESIGN.md section 6 has the two configurations the PSNR study measured (W = 8 with the reference's schedule
for equal steps; iterations, window, interval and horizons / 8 and all learning rates x 8 for equal views).

``--loss_weights {auto,none,file,noise}`` (not a flag of the reference; default auto): per-pixel weights of the training
projections in the image loss (losses.image_loss(..., weights=)): a pixel of weight 0 -- a dead pixel, a panel gap -- is never
used, whatever it holds.  auto: the weights the case records (datagen's ``weights_train``), none for a case that records none,
whose loop is then unchanged; none: ignore them; file: require them; noise: uncertainty.noise_weights of the raw training stack
under the scanner config's noise model, times the recorded weights if there are any.  The FDK initialisation then sees the
projections with their unmeasured pixels filled (weights.fill_unmeasured), ``--save_uncertainty`` the same weights.

``--densify_strategy {threshold,mcmc}`` (not a flag of the reference; default threshold = its loop): mcmc keeps a fixed budget
of Gaussians (mcmc.py, DESIGN.md section 4 "Relocation and position noise"): the densification slot relocates the Gaussians
whose density is not above ``--dead_density`` onto live ones and grows the cloud by 5 % up to ``--cap_max``, every optimiser step
is followed by position noise on the faded Gaussians, and the loss gains L1 penalties on density and scale.  Its defaults are
the original method's numbers and have not been tuned for CT.
"""
import argparse
import os
import os.path as osp
import random
import sys
import time
import uuid

import numpy as np
import torch

from . import losses as FL
from . import metrics as M
from . import model_io
from . import scene as S
from .gaussians import GaussianModel
from .rasterization import GaussianRasterizationSettings, GaussianRasterizer, GaussianRasterizerBatch
from .voxelization import GaussianVoxelizationSettings, GaussianVoxelizer


class OptimizationParams:
    """arguments/__init__.py:44-72."""
    iterations = 30_000
    position_lr_init, position_lr_final, position_lr_max_steps = 0.0002, 0.00002, 30_000
    density_lr_init, density_lr_final, density_lr_max_steps = 0.01, 0.001, 30_000
    scaling_lr_init, scaling_lr_final, scaling_lr_max_steps = 0.005, 0.0005, 30_000
    rotation_lr_init, rotation_lr_final, rotation_lr_max_steps = 0.001, 0.0001, 30_000
    lambda_dssim, lambda_tv, tv_vol_size = 0.25, 0.05, 32
    density_min_threshold = 0.00001
    densification_interval, densify_from_iter, densify_until_iter = 100, 500, 15000
    densify_grad_threshold, densify_scale_threshold = 5.0e-5, 0.1
    max_screen_size, max_scale = None, None
    max_num_gaussians = 500_000
    # opt-in neighbour smoothness of the densities (graph.graph_smoothness, not in the reference): off at 0
    lambda_graph, graph_k, graph_every = 0.0, 8, 100
    # opt-in merging of neighbouring Gaussians (GaussianModel.merge, not in the reference): off at merge_interval 0
    merge_interval, merge_cost, merge_k = 0, 0.1, 8
    merge_from_iter, merge_until_iter = 500, 15000
    # opt-in fixed budget of Gaussians (GaussianModel.relocate / add_noise, not in the reference): off at "threshold".  The
    # numbers, like add_noise's defaults, are the original method's ("3DGS as MCMC"); nobody has tuned them for CT data yet.
    # cap_max None: max_num_gaussians
    densify_strategy = "threshold"
    dead_density, cap_max = 0.005, None
    lambda_density_l1, lambda_scale_l1 = 0.01, 0.01

    def __init__(self, **kw):
        for k, v in kw.items():
            if not hasattr(OptimizationParams, k):
                raise AttributeError(k)
            setattr(self, k, v)


def _bbox(geometry):
    off, s = torch.tensor(geometry["offOrigin"], dtype=torch.float32), torch.tensor(geometry["sVoxel"], dtype=torch.float32)
    return torch.stack([off - s / 2, off + s / 2], 0)


def _query(xyz, dens, scal, rot, center, nVoxel, sVoxel):
    """query() of render_query.py:120-160."""
    vs = GaussianVoxelizationSettings(scale_modifier=1.0, nVoxel_x=int(nVoxel[0]), nVoxel_y=int(nVoxel[1]), nVoxel_z=int(nVoxel[2]),
                                      sVoxel_x=float(sVoxel[0]), sVoxel_y=float(sVoxel[1]), sVoxel_z=float(sVoxel[2]),
                                      center_x=float(center[0]), center_y=float(center[1]), center_z=float(center[2]),
                                      prefiltered=False, debug=False)
    vol, _radii = GaussianVoxelizer(voxel_settings=vs)(means3D=xyz, opacities=dens, scales=scal, rotations=rot, cov3D_precomp=None)
    return vol


def _settings(v, dev, views=None):
    """Rasterizer settings of one view, or of a list of views for GaussianRasterizerBatch ([V,4,4] matrices)."""
    vm = v.world_view_transform if views is None else torch.stack([u.world_view_transform for u in views])
    pm = v.full_proj_transform if views is None else torch.stack([u.full_proj_transform for u in views])
    return GaussianRasterizationSettings(image_height=v.image_height, image_width=v.image_width, tanfovx=v.tanfovx,
                                         tanfovy=v.tanfovy, scale_modifier=1.0, viewmatrix=vm.to(dev), projmatrix=pm.to(dev),
                                         campos=v.camera_center.to(dev), prefiltered=False, mode=v.mode, debug=False)


@torch.no_grad()
def render_views(gaussians, views, dev, batch=8):
    """[V, H, W] projections of the views through GaussianRasterizerBatch, `batch` views per call."""
    xyz, d, s, r = (t.detach() for t in gaussians.activated())
    out = []
    for i in range(0, len(views), batch):
        vb = views[i:i + batch]
        m2d = torch.zeros((len(vb),) + tuple(xyz.shape), dtype=torch.float32, device=dev)
        img, _radii = GaussianRasterizerBatch(_settings(vb[0], dev, vb))(xyz, m2d, d, scales=s, rotations=r)
        out.append(img)
    return torch.cat(out, 0)


@torch.no_grad()
def project_views_exact(gaussians, views, batch=8):
    """[V, H, W] exact line integrals of the model on the views (gaussian_projector.project_gaussians), `batch` views per call."""
    from .gaussian_projector import project_gaussians
    xyz, d, s, r = (t.detach() for t in gaussians.activated())
    return torch.cat([project_gaussians(views[i:i + batch], xyz, d, s, r) for i in range(0, len(views), batch)], 0)


@torch.no_grad()
def evaluate(gaussians, iteration, model_path, geometry, vol_gt, evals, eval_exact=False):
    """training_report of train.py:262-330 without tensorboard: eval2d_<name>.yml per view set, eval3d.yml.  -> eval3d dict.
    eval_exact: also eval2d_<name>_exact.yml, the same metrics on the exact projection of the model instead of the
    rasterizer's image of it."""
    import yaml
    dev = gaussians.device
    path = osp.join(model_path, "eval", "iter_%06d" % iteration)
    os.makedirs(path, exist_ok=True)
    for name, views, gts in evals:
        if not views:
            continue
        renders = [("", render_views(gaussians, views, dev))]
        if eval_exact:
            renders.append(("_exact", project_views_exact(gaussians, views)))
        for suffix, stack in renders:
            images = stack.permute(1, 2, 0)
            psnr_2d, psnr_projs = M.metric_proj(gts, images, "psnr")
            ssim_2d, ssim_projs = M.metric_proj(gts, images, "ssim")
            with open(osp.join(path, "eval2d_%s%s.yml" % (name, suffix)), "w") as f:
                yaml.dump({"psnr_2d": float(psnr_2d), "ssim_2d": float(ssim_2d), "psnr_2d_projs": [float(x) for x in psnr_projs],
                           "ssim_2d_projs": [float(x) for x in ssim_projs]}, f, default_flow_style=False, sort_keys=False)
    xyz, d, s, r = (t.detach() for t in gaussians.activated())
    vol = _query(xyz, d, s, r, geometry["offOrigin"], geometry["nVoxel"], geometry["sVoxel"])
    psnr_3d, ssim_3d, axes = M.metric_vol_both(vol_gt, vol)
    out = {"psnr_3d": float(psnr_3d), "ssim_3d": float(ssim_3d), "ssim_3d_x": float(axes[0]), "ssim_3d_y": float(axes[1]),
           "ssim_3d_z": float(axes[2])}
    with open(osp.join(path, "eval3d.yml"), "w") as f:
        yaml.dump(out, f, default_flow_style=False, sort_keys=False)
    return out


@torch.no_grad()
def write_uncertainty(gaussians, views, geometry, path, prior_precision, batch=8, weights=None):
    """fisher.npz (xyz [P,3], density [P,1], scaling [P,3], rotation [P,4]: the Fisher diagonal of the activated parameters
    over `views` with unit weights, or with `weights`: one [H, W] device tensor per view; `batch` views per launch) and
    vol_std.npy ([nx, ny, nz]: the square root of the field's predictive variance at the voxel centres of the evaluation
    grid, under the Laplace variances 1 / (F + prior_precision)) into `path`."""
    from . import uncertainty as U
    from .field import voxel_centres
    xyz, d, s, r = (t.detach() for t in gaussians.activated())
    F = None
    for i in range(0, len(views), batch):
        Fi = U.fisher_diagonal(views[i:i + batch], xyz, d, s, r,
                               None if weights is None else torch.stack(list(weights[i:i + batch])))
        F = Fi if F is None else U.CloudTuple(*(a + b for a, b in zip(F, Fi)))
    var = U.parameter_variance(F, prior_precision)
    pts = voxel_centres(geometry["offOrigin"], geometry["nVoxel"], geometry["sVoxel"], xyz.device)
    std = U.field_variance(pts, xyz, d, s, r, var).sqrt()
    os.makedirs(path, exist_ok=True)
    np.savez(osp.join(path, "fisher.npz"), **{k: v.cpu().numpy() for k, v in F._asdict().items()})
    np.save(osp.join(path, "vol_std.npy"), std.cpu().numpy())


def render_loss_batch(gaussians, views, gts, lambda_dssim, dev, weights=None):
    """The image term of a step on several views: ONE GaussianRasterizerBatch call on `views` (scene.View list) and ONE
    losses.image_loss_batch node against `gts` (their ground truths, [H, W] device tensors), weighted per pixel by `weights`
    (None, or the views' [H, W] device tensors).
    -> (loss: the mean over the views, radii [W, P], screen [W, P, 3]: the leaf whose .grad the backward fills with every
    view's dL/dmeans2D of that mean loss)."""
    xyz, dens, scal, rot = gaussians.activated()
    screen = torch.zeros((len(views),) + tuple(xyz.shape), dtype=torch.float32, device=dev, requires_grad=True)
    img, radii = GaussianRasterizerBatch(_settings(views[0], dev, views))(means3D=xyz, means2D=screen, opacities=dens, scales=scal,
                                                                          rotations=rot, cov3D_precomp=None)
    loss, _parts = FL.image_loss_batch(img, gts, lambda_dssim, weights)
    return loss, radii, screen


def pick_views(stack, n_views, count, rng):
    """The next `count` training views (train.py:104-106 per view): each is popped from `stack` at a position drawn from
    `rng` (random.Random), and the stack is refilled with 0 .. n_views - 1 whenever it runs empty -- also in the middle of a
    step.  `stack` is updated in place.  -> list of view indices."""
    picked = []
    for _ in range(count):
        if not stack:
            stack.extend(range(n_views))
        picked.append(stack.pop(rng.randint(0, len(stack) - 1)))
    return picked


def training(train_views, train_projs, test_views, test_projs, vol_gt, geometry, init_points, opt, model_path,
             scale_bound=None, test_iterations=(), save_iterations=(), checkpoint_iterations=(), start_checkpoint=None,
             seed=0, log=print, device="cuda", views_per_step=1, eval_exact=False, save_uncertainty=None, train_weights=None,
             save_mesh=None, save_render=None):
    """The training loop of train.py:34-216.  views: scene.View lists; projections: [V, H, W] in scene units (times
    scene_scale); vol_gt [nx, ny, nz]; geometry: the NORMALISED scanner config (nVoxel, sVoxel, offOrigin, dVoxel);
    init_points [N, 4] = xyz | density; scale_bound: (lo, hi) in scene units or None.  Randomness (view order, TV patch centres,
    split samples) comes from generators seeded with `seed`: random.Random for the view order, a CPU torch.Generator for the
    rest, in the order tests/mini_trainer.py draws them.
    views_per_step = W > 1: an iteration is one optimiser step on W views (pick_views) through GaussianRasterizerBatch,
    losses.image_loss_batch (the MEAN over the views, so the parameter gradients are the views' mean) plus ONE TV patch, and
    one batched statistics call with grad_scale = W: the statistics see every view's own screen-space gradient, which keeps
    densify_grad_threshold a per-view quantity whatever W is.  W = 1 is the single-view loop, unchanged.
    eval_exact: every evaluation also writes eval2d_<name>_exact.yml (evaluate); training itself is untouched.
    save_uncertainty = lambda > 0 (None: off): after the last iteration ``save_uncertainty`` writes fisher.npz and vol_std.npy
    into the last point_cloud/iteration_N; training itself is untouched.
    save_mesh = level (None: off, mesh.py is then never imported): after the last iteration ``mesh.model_isosurface`` of the
    final model at that level, on the evaluation grid, snapped onto the field and closed at the grid's border, goes into
    mesh.ply next to the predicted volume (scene units, with normals); training itself is untouched.
    save_render = (H, W) (None: off, volume_render.py is then never imported): after the last iteration the final model's
    volume on the evaluation grid goes through ``volume_render.picture`` at its defaults (plot_volume.py's half-cut viridis
    view) into render.png next to the predicted volume; training itself is untouched.
    opt.lambda_graph > 0 (absent = 0: off, the loop is then the one above and graph.py is never called): the loss gains
    lambda_graph * graph.graph_smoothness(density[:, 0], G, kind="l1"), G = the opt.graph_k (8) nearest neighbours of
    xyz.detach(), rebuilt every opt.graph_every (100) iterations and whenever the number of Gaussians changed.
    opt.merge_interval = N > 0 (absent = 0: off, the loop is then the one above and merge.py is never imported): every N-th
    iteration with opt.merge_from_iter < iteration < opt.merge_until_iter, right after the densification slot,
    gaussians.merge(opt.merge_cost, k=opt.merge_k) replaces neighbouring Gaussians that say the same thing by one.
    train_weights (None: off, the loop is then the one above): per-pixel weights of the training projections, [H, W] shared by
    the views or [V, H, W] (weights.resolve_weights): the image term becomes the weighted loss of losses.image_loss /
    image_loss_batch, in which a pixel whose weight is not > 0 is never used (train_projs may hold anything there, NaN
    included), and save_uncertainty weighs the Fisher diagonal with them.  The evaluation metrics stay unweighted.
    opt.densify_strategy = "mcmc" (absent = "threshold": the loop is then the one above and mcmc.py is never imported): the
    densification slot calls gaussians.relocate(iteration, opt.dead_density, opt.cap_max or opt.max_num_gaussians, seed=seed)
    instead of densify_and_prune; every step() is followed by gaussians.add_noise(iteration, seed=seed) at its defaults; and
    the loss gains opt.lambda_density_l1 * density.mean() + opt.lambda_scale_l1 *
    scaling.mean() on the activated leaves.  The generator is keyed by (seed, iteration): a resumed run draws what the
    uninterrupted one would.
    -> dict(model, evals {iteration: eval3d}, it_per_s, views_per_s, P, graph_builds, merged_pairs, relocations)."""
    W = int(views_per_step)
    if W < 1:
        raise ValueError("views_per_step must be >= 1, got %r" % (views_per_step,))
    if save_uncertainty is not None and not float(save_uncertainty) > 0:
        raise ValueError("save_uncertainty must be a positive prior precision, got %r" % (save_uncertainty,))
    dev = torch.device(device)
    gaussians = GaussianModel(scale_bound, device=dev)
    gaussians.create_from_pcd(init_points[:, :3], init_points[:, 3:4], 1.0)
    gaussians.training_setup(opt)
    first_iter = 0
    if start_checkpoint:
        model_params, first_iter = torch.load(start_checkpoint, map_location=dev, weights_only=False)
        gaussians.restore(model_params, opt)
        log("Load checkpoint %s." % osp.basename(start_checkpoint))
    bbox = _bbox(geometry)
    volume_to_world = max(geometry["sVoxel"])
    max_scale = opt.max_scale * volume_to_world if opt.max_scale else None
    densify_scale_threshold = opt.densify_scale_threshold * volume_to_world if opt.densify_scale_threshold else None
    gts = [torch.as_tensor(np.asarray(p), dtype=torch.float32).to(dev) for p in train_projs]
    wts = None
    if train_weights is not None:
        w = np.asarray(train_weights, dtype=np.float32)
        if w.shape != tuple(gts[0].shape) and w.shape != (len(gts),) + tuple(gts[0].shape):
            raise ValueError("train_weights is %s but the training projections are %s" % (w.shape, (len(gts),) + tuple(gts[0].shape)))
        with np.errstate(invalid="ignore"):
            w = torch.from_numpy(np.where(w > 0, w, np.float32(0))).to(dev)
        wts = [w] * len(gts) if w.dim() == 2 else list(w)
    vol_gt = torch.as_tensor(np.asarray(vol_gt), dtype=torch.float32).to(dev)
    evals = [("render_train", train_views, torch.stack(gts, -1)),
             ("render_test", test_views,
              torch.as_tensor(np.asarray(test_projs), dtype=torch.float32).to(dev).permute(1, 2, 0) if len(test_views) else None)]
    use_tv = opt.lambda_tv > 0
    lambda_graph = float(getattr(opt, "lambda_graph", OptimizationParams.lambda_graph))
    graph_k = int(getattr(opt, "graph_k", OptimizationParams.graph_k))
    graph_every = int(getattr(opt, "graph_every", OptimizationParams.graph_every))
    if lambda_graph > 0 and graph_every < 1:
        raise ValueError("graph_every must be >= 1, got %r" % (graph_every,))
    nbr_graph = None
    if lambda_graph > 0:
        from . import graph as NG
    merge_interval = int(getattr(opt, "merge_interval", OptimizationParams.merge_interval))
    merge_cost = float(getattr(opt, "merge_cost", OptimizationParams.merge_cost))
    merge_k = int(getattr(opt, "merge_k", OptimizationParams.merge_k))
    merge_from = int(getattr(opt, "merge_from_iter", OptimizationParams.merge_from_iter))
    merge_until = int(getattr(opt, "merge_until_iter", OptimizationParams.merge_until_iter))
    if merge_interval < 0:
        raise ValueError("merge_interval must be >= 0, got %r" % (merge_interval,))
    strategy = getattr(opt, "densify_strategy", OptimizationParams.densify_strategy)
    if strategy not in ("threshold", "mcmc"):
        raise ValueError("densify_strategy must be 'threshold' or 'mcmc', got %r" % (strategy,))
    mcmc = strategy == "mcmc"
    if mcmc:
        dead_density = float(getattr(opt, "dead_density", OptimizationParams.dead_density))
        cap_max = getattr(opt, "cap_max", None)
        cap_max = int(opt.max_num_gaussians if cap_max is None else cap_max)
        lambda_density_l1 = float(getattr(opt, "lambda_density_l1", OptimizationParams.lambda_density_l1))
        lambda_scale_l1 = float(getattr(opt, "lambda_scale_l1", OptimizationParams.lambda_scale_l1))
    tvN = torch.tensor([opt.tv_vol_size] * 3)
    tvS = torch.tensor(geometry["dVoxel"], dtype=torch.float32) * tvN
    settings = [_settings(v, dev) for v in train_views]
    gen = torch.Generator().manual_seed(seed)
    pyrng = random.Random(seed)
    ckpt_path = osp.join(model_path, "ckpt")
    os.makedirs(ckpt_path, exist_ok=True)
    out = {"evals": {}, "graph_builds": 0, "merged_pairs": 0, "relocations": 0}
    if first_iter == 0 and 0 in test_iterations:
        out["evals"][0] = evaluate(gaussians, 0, model_path, geometry, vol_gt, evals, eval_exact)
    stack = []
    t_train, n_timed = 0.0, 0
    for iteration in range(first_iter + 1, opt.iterations + 1):
        t0 = time.perf_counter()
        gaussians.update_learning_rate(iteration)
        picked = pick_views(stack, len(train_views), W, pyrng)
        xyz, dens, scal, rot = gaussians.activated()
        if W == 1:
            vi = picked[0]
            screen = torch.zeros_like(xyz, requires_grad=True)
            img, radii = GaussianRasterizer(raster_settings=settings[vi])(means3D=xyz, means2D=screen, opacities=dens,
                                                                          scales=scal, rotations=rot, cov3D_precomp=None)
            loss, _parts = FL.image_loss(img, gts[vi], opt.lambda_dssim, None if wts is None else wts[vi])
        else:
            loss, radii, screen = render_loss_batch(gaussians, [train_views[vi] for vi in picked], [gts[vi] for vi in picked],
                                                    opt.lambda_dssim, dev, None if wts is None else [wts[vi] for vi in picked])
        if use_tv:
            c = (bbox[0] + tvS / 2) + (bbox[1] - tvS - bbox[0]) * torch.rand(3, generator=gen)
            loss = loss + opt.lambda_tv * FL.tv_3d_loss(_query(xyz, dens, scal, rot, c, tvN, tvS))
        if lambda_graph > 0:
            if nbr_graph is None or nbr_graph.P != xyz.shape[0] or iteration % graph_every == 0:
                nbr_graph = NG.knn_graph(xyz.detach(), graph_k)
                out["graph_builds"] += 1
            loss = loss + lambda_graph * NG.graph_smoothness(dens[:, 0], nbr_graph, kind="l1")
        if mcmc:   # the penalties that let Gaussians die: L1 on the activated densities and scales
            loss = loss + lambda_density_l1 * dens.mean() + lambda_scale_l1 * scal.mean()
        loss.backward()
        with torch.no_grad():
            gaussians.add_densification_stats(radii, screen.grad, grad_scale=float(W))
            if opt.densify_from_iter < iteration < opt.densify_until_iter and iteration % opt.densification_interval == 0:
                if mcmc:
                    gaussians.relocate(iteration, dead_density, cap_max, seed=seed)
                    out["relocations"] += 1
                else:
                    gaussians.densify_and_prune(opt.densify_grad_threshold, opt.density_min_threshold, opt.max_screen_size,
                                                max_scale, opt.max_num_gaussians, densify_scale_threshold, bbox,
                                                normals=torch.randn((2, gaussians.P, 3), generator=gen))
            if merge_interval > 0 and merge_from < iteration < merge_until and iteration % merge_interval == 0:
                out["merged_pairs"] += gaussians.merge(merge_cost, k=merge_k)
            if iteration < opt.iterations:
                gaussians.step()
                if mcmc:
                    gaussians.add_noise(iteration, seed=seed)
            else:
                for t in gaussians.activated():
                    t.grad = None
        torch.cuda.synchronize(dev)
        t_train += time.perf_counter() - t0
        n_timed += 1
        if iteration in save_iterations or iteration == opt.iterations:
            pc = osp.join(model_path, "point_cloud", "iteration_%d" % iteration)
            gaussians.save_ply(osp.join(pc, "point_cloud.pickle"))
            with torch.no_grad():
                x, d, s, r = (t.detach() for t in gaussians.activated())
                vol = _query(x, d, s, r, geometry["offOrigin"], geometry["nVoxel"], geometry["sVoxel"])
            model_io.save_volumes(pc, vol_gt, vol)
        if iteration in checkpoint_iterations:
            model_io.save_checkpoint(osp.join(ckpt_path, "chkpnt%d.pth" % iteration), gaussians.capture(), iteration)
        if iteration in test_iterations:
            out["evals"][iteration] = e = evaluate(gaussians, iteration, model_path, geometry, vol_gt, evals, eval_exact)
            log("[ITER %d] Evaluating: psnr3d %.3f, ssim3d %.3f, P %d" % (iteration, e["psnr_3d"], e["ssim_3d"], gaussians.P))
    if save_uncertainty is not None:
        write_uncertainty(gaussians, train_views, geometry, osp.join(model_path, "point_cloud", "iteration_%d" % opt.iterations),
                          float(save_uncertainty), weights=wts)
    if save_mesh is not None:
        from . import mesh as MS
        with torch.no_grad():
            x, d, s, r = (t.detach() for t in gaussians.activated())
            mv, mf, mn = MS.model_isosurface(x, d, s, r, float(save_mesh), geometry["offOrigin"], geometry["nVoxel"],
                                             geometry["sVoxel"])
        MS.write_ply(osp.join(model_path, "point_cloud", "iteration_%d" % opt.iterations, "mesh.ply"), mv, mf, mn)
        log("mesh.ply: %d vertices, %d triangles at level %g" % (mv.shape[0], mf.shape[0], float(save_mesh)))
    if save_render is not None:
        from . import volume_render as VR
        with torch.no_grad():
            x, d, s, r = (t.detach() for t in gaussians.activated())
            vol = _query(x, d, s, r, geometry["offOrigin"], geometry["nVoxel"], geometry["sVoxel"])
            img = VR.picture(vol, geometry["sVoxel"], geometry["offOrigin"], size=save_render)[0]
        VR.write_png(osp.join(model_path, "point_cloud", "iteration_%d" % opt.iterations, "render.png"), img)
        log("render.png: %d x %d" % (img.shape[1], img.shape[0]))
    out["it_per_s"] = n_timed / t_train if t_train > 0 else float("nan")
    out["views_per_s"] = W * out["it_per_s"]
    out["model"] = gaussians
    out["P"] = gaussians.P
    log("Training complete: %d iterations, %s, %d Gaussians" % (n_timed, _rate(out, W), gaussians.P))
    return out


def _rate(out, W):
    """'N it/s', for several views per step followed by 'N views/s'."""
    return "%.1f it/s" % out["it_per_s"] + (", %.1f views/s" % out["views_per_s"] if W > 1 else "")


# ---------------------------------------------------------------------------------------------- the case on disk
def load_case(source_path, ply_path="", seed=0, loss_weights="none"):
    """Scene + initialize_gaussian for a case in datagen's layout: the views (scene.make_view on the raw config), the
    projections times scene_scale, the normalised geometry (dataset_readers.py:62-76), and the initial points from
    ``init_<case>.npy``, else `ply_path` (.npy), else fdk.init_pcd on the normalised scene.
    loss_weights: a mode of weights.resolve_weights; its result is ``train_weights`` (None for "none", and for "auto" on a case
    that records no weights: weights.py is then not imported), and with weights the FDK initialisation reads the training
    projections with their unmeasured pixels filled (weights.fill_unmeasured)."""
    from . import fdk
    from .recon import _read_case
    case = _read_case(source_path)
    cfg, scale = case["cfg"], case["scale"]
    geo = dict(cfg)
    geo.setdefault("dVoxel", list(np.array(cfg["sVoxel"]) / np.array(cfg["nVoxel"])))
    geo.setdefault("dDetector", list(np.array(cfg["sDetector"]) / np.array(cfg["nDetector"])))
    for k in ("dVoxel", "sVoxel", "sDetector", "dDetector", "offOrigin", "offDetector", "DSD", "DSO"):
        if k in geo:
            geo[k] = (np.array(geo[k]) * scale).tolist()
    det = tuple(int(x) for x in cfg["nDetector"])
    out = {"geometry": geo, "vol_gt": case["vol"], "scale": scale, "train_weights": None}
    if loss_weights != "none" and (loss_weights != "auto" or case["weights_train"] is not None):
        from . import weights as WT
        out["train_weights"] = WT.resolve_weights(case, loss_weights)
    for split in ("train", "test"):
        projs, angles = case[split]
        out[split + "_views"] = [S.make_view(a, det, cfg) for a in angles]
        out[split + "_projs"] = projs * np.float32(scale)
    init = osp.join(source_path, "init_" + osp.basename(osp.normpath(source_path)) + ".npy")
    if not ply_path and osp.exists(init):
        out["init_points"] = np.load(init)
    elif ply_path:
        if not ply_path.endswith(".npy"):
            raise ValueError("--ply_path: only .npy point clouds (xyz | density) are read")
        out["init_points"] = np.load(ply_path)
    else:
        projs, angles = case["train"]
        if out["train_weights"] is not None:
            projs = WT.fill_unmeasured(projs, out["train_weights"])
        projs = projs * np.float32(scale)
        # initialize_pcd.py's 50000 points, or every voxel above its threshold in a smaller reconstruction
        n_points = min(50000, int((fdk.recon_volume(projs, angles, geo) > 0.05).sum()))
        out["init_points"] = fdk.init_pcd(projs, angles, geo, n_points=n_points, rng=np.random.RandomState(seed))
    return out


def build_parser():
    """The reference's flags (arguments/__init__.py, train.py:376-389)."""
    ap = argparse.ArgumentParser(description="Training script parameters")
    g = ap.add_argument_group("Loading Parameters")
    g.add_argument("--source_path", "-s", default="", type=str)
    g.add_argument("--model_path", "-m", default="", type=str)
    g.add_argument("--data_device", default="cuda", type=str)
    g.add_argument("--ply_path", default="", type=str)
    g.add_argument("--scale_min", default=0.0005, type=float)
    g.add_argument("--scale_max", default=0.5, type=float)
    g.add_argument("--eval", default=True, action="store_true")
    g = ap.add_argument_group("Optimization Parameters")
    for k, v in vars(OptimizationParams).items():
        if k.startswith("_") or callable(v):
            continue
        if k == "densify_strategy":
            g.add_argument("--" + k, default=v, choices=("threshold", "mcmc"),
                           help="threshold: the reference's clone / split / prune.  mcmc: a fixed budget -- the densification slot "
                                "relocates Gaussians whose density is not above --dead_density onto live ones and grows the cloud by "
                                "5 %% up to --cap_max (default: max_num_gaussians), every step adds position noise to faded Gaussians, "
                                "and the loss gains --lambda_density_l1 / --lambda_scale_l1 times the mean density / scale.  Its "
                                "defaults are the original method's, untuned for CT")
            continue
        g.add_argument("--" + k, default=v, type=float if v is None else type(v))
    g = ap.add_argument_group("Pipeline Parameters")
    g.add_argument("--compute_cov3D_python", default=False, action="store_true")
    g.add_argument("--debug", default=False, action="store_true")
    ap.add_argument("--detect_anomaly", action="store_true", default=False)
    ap.add_argument("--test_iterations", nargs="+", type=int, default=[5_000, 10_000, 20_000])
    ap.add_argument("--save_iterations", nargs="+", type=int, default=[])
    ap.add_argument("--quiet", action="store_true")
    ap.add_argument("--checkpoint_iterations", nargs="+", type=int, default=[])
    ap.add_argument("--start_checkpoint", type=str, default=None)
    ap.add_argument("--config", type=str, default=None)
    ap.add_argument("--views_per_step", type=int, default=1,
                    help="views per optimiser step: one batched render, one batched loss and one batched statistics launch per "
                         "step.  --iterations, the densification window and the *_lr_max_steps then count optimiser steps, and "
                         "the learning rates are NOT rescaled.  Measured (DESIGN.md section 6): 8 with the default schedule "
                         "gains 3.6 dB of 3D PSNR at equal steps; for equal views divide iterations, densification window and "
                         "interval and *_lr_max_steps by 8 and multiply the eight *_lr_init / *_lr_final by 8 (+0.48 dB)")
    ap.add_argument("--eval_exact", action="store_true", default=False,
                    help="every evaluation also writes eval2d_render_{train,test}_exact.yml: the 2D metrics on the exact line "
                         "integrals of the model (gaussian_projector) next to those on the rasterizer's image of it")
    ap.add_argument("--loss_weights", choices=("auto", "none", "file", "noise"), default="auto",
                    help="per-pixel weights of the training projections in the image loss (a weight of 0 excludes the pixel, "
                         "whatever it holds): auto = the case's recorded weights_train if it has any, none = ignore them, file = "
                         "require them, noise = the inverse variances of the scanner config's noise model (uncertainty.noise_weights "
                         "on the raw training stack), times the recorded weights if any")
    ap.add_argument("--save_uncertainty", type=float, default=None, metavar="LAMBDA",
                    help="after the last iteration write fisher.npz (the Fisher diagonal of the activated parameters over the "
                         "training views, unit weights or those of --loss_weights) and vol_std.npy (the standard deviation of the field on the evaluation "
                         "grid under the Laplace variances 1 / (F + LAMBDA)) into the last point_cloud/iteration_N")
    ap.add_argument("--save_mesh", type=float, default=None, metavar="LEVEL",
                    help="after the last iteration write mesh.ply into the last point_cloud/iteration_N: the isosurface of the "
                         "final model's density at LEVEL (scene units), extracted on the evaluation grid, moved onto the "
                         "continuous field's level set and closed at the grid's border (mesh.model_isosurface)")
    ap.add_argument("--save_render", type=int, nargs=2, default=None, metavar=("H", "W"),
                    help="after the last iteration write render.png, H rows by W columns, into the last "
                         "point_cloud/iteration_N: the final model's volume on the evaluation grid by direct volume rendering "
                         "at the defaults of volume_render.py (half cut away along x, viridis, linear opacity)")
    return ap


def main(argv=None):
    ap = build_parser()
    args = ap.parse_args(sys.argv[1:] if argv is None else argv)
    if args.config is not None:
        import yaml
        with open(args.config) as f:
            cfg = yaml.safe_load(f)
        for k, v in cfg.items():
            if not hasattr(args, k):
                ap.error("unknown key %r in %s" % (k, args.config))
            setattr(args, k, v)
    if args.views_per_step < 1:
        ap.error("--views_per_step must be >= 1")
    if args.save_uncertainty is not None and not args.save_uncertainty > 0:
        ap.error("--save_uncertainty needs a positive prior precision")
    if args.compute_cov3D_python:
        ap.error("--compute_cov3D_python is not supported: the kernels build the covariance from scales and rotations")
    args.save_iterations.append(args.iterations)
    args.test_iterations += [args.iterations, 1]
    if not args.source_path:
        ap.error("--source_path is required")
    if not args.model_path:
        args.model_path = osp.join("./output/", str(uuid.uuid4())[0:10])
    os.makedirs(args.model_path, exist_ok=True)
    print("Optimizing " + args.model_path)
    torch.autograd.set_detect_anomaly(args.detect_anomaly)
    try:
        case = load_case(args.source_path, args.ply_path, loss_weights=args.loss_weights)
    except ValueError as e:
        if "--loss_weights" not in str(e):
            raise
        ap.error(str(e))
    volume_to_world = max(case["geometry"]["sVoxel"])
    scale_bound = None
    if args.scale_min > 0 and args.scale_max > 0:
        scale_bound = np.array([args.scale_min, args.scale_max]) * volume_to_world
    opt = OptimizationParams(**{k: getattr(args, k) for k in vars(OptimizationParams) if not k.startswith("_") and
                                not callable(getattr(OptimizationParams, k))})
    log = (lambda *a: None) if args.quiet else print
    out = training(case["train_views"], case["train_projs"], case["test_views"], case["test_projs"], case["vol_gt"],
                   case["geometry"], case["init_points"], opt, args.model_path, scale_bound, set(args.test_iterations),
                   set(args.save_iterations), set(args.checkpoint_iterations), args.start_checkpoint, log=log,
                   views_per_step=args.views_per_step, eval_exact=args.eval_exact, save_uncertainty=args.save_uncertainty,
                   train_weights=case["train_weights"], save_mesh=args.save_mesh, save_render=args.save_render)
    print("Training complete. " + _rate(out, args.views_per_step))
    return out


if __name__ == "__main__":
    main()
