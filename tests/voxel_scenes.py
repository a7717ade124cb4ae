"""Seeded voxelizer scenes at the edges of the render's tiers (tests/test_voxel_tiers_gpu.py, tests/test_voxel_ref_cpu.py).

Every scene is a scene.Cloud and the grids it is rendered on, (nVoxel, sVoxel, center): grids of at most 64 tiles go through the
small-grid path, larger ones through the stick-first and the general chain.  Scales are world-isotropic unless a scene says
otherwise and are clamped to the reference's bound [0.0005, 0.5] * extent (extent 2.0, the scanner's volume).
"""
from typing import NamedTuple

import numpy as np
import torch

from r2_gaussian_amd import scene as S

EXTENT = 2.0
SMIN, SMAX = 0.0005 * EXTENT, 0.5 * EXTENT


class Scene(NamedTuple):
    name: str
    cloud: S.Cloud
    grids: list        # [(nVoxel, sVoxel, center)]


def _quats(rng, n):
    q = rng.normal(size=(n, 4))
    return q / np.linalg.norm(q, axis=1, keepdims=True)


def _cloud(xyz, scales, q, density):
    t = lambda a, *s: torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float32).reshape(*s)))   # noqa: E731
    n = len(xyz)
    return S.Cloud(t(xyz, n, 3), t(np.clip(scales, SMIN, SMAX), n, 3), t(q, n, 4), t(density, n, 1))


def _cat(*clouds):
    return S.Cloud(*(torch.cat([getattr(c, f) for c in clouds], 0).contiguous() for f in S.Cloud._fields))


def _needles_and_pancakes(rng, n, dv, lo, hi, long_cap, free_frac=0.02):
    """n Gaussians, half needles (one long axis), half pancakes (one short axis); short axis log-uniform in [lo, hi] voxels,
    long / short log-uniform in [1, 1000], the long axis capped at long_cap voxels except for a fraction free_frac (up to the bound)."""
    short = np.exp(rng.uniform(np.log(lo), np.log(hi), n))
    ratio = np.exp(rng.uniform(0.0, np.log(1000.0), n))
    free = rng.random(n) < free_frac
    longer = np.where(free, short * ratio, np.minimum(short * ratio, long_cap))
    needle = rng.random(n) < 0.5
    s = np.where(needle[:, None], np.stack([longer, short, short], 1), np.stack([longer, longer, short], 1))
    return s * dv, _quats(rng, n)


def tier_scene():
    """Needles and pancakes on both sides of needs_exact_slab3, in one volume."""
    rng = np.random.default_rng(101)
    n = 400
    dv = 2.0 / 64
    xyz = rng.uniform(-0.85, 0.85, (n, 3))
    sc, q = _needles_and_pancakes(rng, n, dv, 0.05, 2.0, 4.0)
    rho = np.exp(rng.uniform(np.log(0.004), np.log(0.06), n))
    return Scene("tier", _cloud(xyz, sc, q, rho),
                 [((64, 64, 64), (2.0, 2.0, 2.0), (0.0, 0.0, 0.0)), ((32, 32, 32), (1.0, 1.0, 1.0), (0.1, -0.05, 0.0))])


def subvoxel_scene():
    """sigma 0.05 - 0.4 voxel; a quarter centred on voxel corners with sigma <= 0.1, which reach no voxel centre at all."""
    rng = np.random.default_rng(102)
    n = 6000
    dv = 2.0 / 64
    pv = rng.uniform(2.0, 62.0, (n, 3))
    corner = rng.random(n) < 0.25
    pv[corner] = np.round(pv[corner])
    sig = np.exp(rng.uniform(np.log(0.05), np.log(0.4), (n, 3)))
    sig[corner] = np.minimum(sig[corner], 0.1)
    xyz = pv * dv - 1.0
    rho = rng.uniform(0.05, 0.9, n)
    return Scene("subvoxel", _cloud(xyz, sig * dv, _quats(rng, n), rho),
                 [((64, 64, 64), (2.0, 2.0, 2.0), (0.0, 0.0, 0.0)), ((32, 32, 32), (1.0, 1.0, 1.0), (0.0, 0.0, 0.0))])


def opacity_scene():
    """Peak densities within +-1 % of 1e-6 (half of them centred exactly on a voxel centre), below 1e-6, and from 1 to 50."""
    rng = np.random.default_rng(103)
    n = 4000
    dv = 2.0 / 64
    pv = rng.uniform(3.0, 61.0, (n, 3))
    cls = rng.choice(4, n, p=[0.3, 0.2, 0.01, 0.49])   # near the cut-off, below it, 1..50, ordinary
    on_centre = (cls == 0) & (rng.random(n) < 0.5)
    pv[on_centre] = np.floor(pv[on_centre]) + 0.5
    rho = np.where(cls == 0, 1e-6 * rng.uniform(0.99, 1.01, n),
                   np.where(cls == 1, np.exp(rng.uniform(np.log(1e-9), np.log(0.999e-6), n)),
                            np.where(cls == 2, np.exp(rng.uniform(0.0, np.log(50.0), n)), rng.uniform(0.005, 0.05, n))))
    sig = np.exp(rng.uniform(np.log(0.4), np.log(2.5), (n, 3)))
    return Scene("opacity", _cloud(pv * dv - 1.0, sig * dv, _quats(rng, n), rho),
                 [((64, 64, 64), (2.0, 2.0, 2.0), (0.0, 0.0, 0.0)), ((32, 32, 32), (1.0, 1.0, 1.0), (0.0, 0.0, 0.0))])


def aniso_scene():
    """Voxels of 0.02 x 0.08 x 0.01 (8 : 1), one voxel thick along y: world-isotropic Gaussians are thin in y, long in z."""
    rng = np.random.default_rng(104)
    n = 800
    xyz = np.stack([rng.uniform(-1.0, 1.0, n), rng.uniform(-0.12, 0.12, n), rng.uniform(-1.0, 1.0, n)], 1)
    s = np.exp(rng.uniform(np.log(0.004), np.log(0.025), n))
    sc = s[:, None] * np.exp(rng.uniform(-0.3, 0.3, (n, 3)))
    rho = rng.uniform(0.02, 0.6, n)
    return Scene("aniso", _cloud(xyz, sc, _quats(rng, n), rho),
                 [((100, 1, 200), (2.0, 0.08, 2.0), (0.0, 0.0, 0.0)), ((40, 1, 60), (0.8, 0.08, 0.6), (0.1, 0.01, -0.2))])


def faces_scene():
    """Centres outside the volume whose supports cross its faces; centres exactly on voxel centres and on tile boundaries.
    (Voxel size 1/32 on both grids: the world coordinates below map to those voxel coordinates exactly.)"""
    rng = np.random.default_rng(105)
    dv = 2.0 / 64
    n_out, n_ctr, n_tile = 1500, 1000, 1000
    pv = rng.uniform(0.0, 64.0, (n_out, 3))
    ax = rng.integers(0, 3, n_out)
    side = rng.random(n_out) < 0.5
    pv[np.arange(n_out), ax] = np.where(side, -rng.uniform(0.05, 5.0, n_out), 64.0 + rng.uniform(0.05, 5.0, n_out))
    pc = rng.integers(0, 64, (n_ctr, 3)) + 0.5
    pt = rng.integers(0, 9, (n_tile, 3)) * 8.0
    pv = np.concatenate([pv, pc, pt], 0)
    n = len(pv)
    sig = np.exp(rng.uniform(np.log(0.3), np.log(3.0), (n, 3)))
    rho = rng.uniform(0.005, 0.1, n)
    return Scene("faces", _cloud(pv * dv - 1.0, sig * dv, _quats(rng, n), rho),
                 [((64, 64, 64), (2.0, 2.0, 2.0), (0.0, 0.0, 0.0)), ((32, 32, 32), (1.0, 1.0, 1.0), (0.0, 0.0, 0.0))])


def lists_scene():
    """Tile lists of every length: a dense cluster (lists of 300 - 900: several staging batches and the carry), a medium band and
    a sparse rest (lists under 25: the short-list kernel)."""
    rng = np.random.default_rng(106)
    dv = 2.0 / 64
    dense = rng.normal(0.0, 1.0, (900, 3)) + np.array([20.0, 20.0, 20.0])
    medium = rng.uniform(8.0, 56.0, (800, 3))
    sparse = rng.uniform(0.0, 64.0, (800, 3))
    pv = np.concatenate([dense, medium, sparse], 0)
    n = len(pv)
    sig = np.exp(rng.uniform(np.log(0.4), np.log(2.0), (n, 3)))
    sig[:900] = np.exp(rng.uniform(np.log(0.3), np.log(1.0), (900, 3)))
    rho = rng.uniform(0.005, 0.1, n)
    return Scene("lists", _cloud(pv * dv - 1.0, sig * dv, _quats(rng, n), rho),
                 [((64, 64, 64), (2.0, 2.0, 2.0), (0.0, 0.0, 0.0)), ((32, 32, 32), (1.0, 1.0, 1.0), (-0.5, -0.5, -0.5))])


def big_scene():
    """The 256^3 query on a mixed cloud: needles, pancakes, sub-voxel and ordinary Gaussians (sampled voxels only)."""
    rng = np.random.default_rng(107)
    dv = 2.0 / 256
    n1, n2 = 10000, 6000
    sc1, q1 = _needles_and_pancakes(rng, n1, dv, 0.1, 3.0, 8.0, free_frac=0.002)
    sc2 = np.exp(rng.uniform(np.log(0.1), np.log(4.0), (n2, 3))) * dv
    xyz = rng.uniform(-0.95, 0.95, (n1 + n2, 3))
    rho = np.exp(rng.uniform(np.log(0.002), np.log(0.04), n1 + n2))
    return Scene("big256", _cloud(xyz, np.concatenate([sc1, sc2]), np.concatenate([q1, _quats(rng, n2)]), rho),
                 [((256, 256, 256), (2.0, 2.0, 2.0), (0.0, 0.0, 0.0))])


SCENES = {f.__name__[:-6]: f for f in (tier_scene, subvoxel_scene, opacity_scene, aniso_scene, faces_scene, lists_scene)}
