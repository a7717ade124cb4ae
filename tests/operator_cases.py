"""What the GPU tests of the volume operator pairs share (test_recon_gpu.py: the interpolated pair, test_siddon_gpu.py: the
Siddon pair): the transpose geometries, the tiny scanner of the algorithm tests and its right-hand side, and the dense
matrices of both directions from one-hot operands."""
import numpy as np
import torch

from r2_gaussian_amd import projector as K
from r2_gaussian_amd import scene as S

# name, scanner, (H, W), nVoxel, sVoxel, center, angles, accuracy
TRANSPOSE = [
    ("cone_aniso_offset", S.CONE_BEAM, (11, 13), (9, 7, 8), (1.8, 1.4, 1.7), (0.1, -0.05, 0.07), (0.3, 2.1, 4.0), 0.5),
    ("parallel_aniso_offset", S.PARALLEL_BEAM, (11, 13), (9, 7, 8), (1.8, 1.4, 1.7), (0.1, -0.05, 0.07), (0.3, 2.1, 4.0), 0.5),
    ("cone_misses", S.CONE_BEAM, (11, 13), (9, 7, 8), (0.6, 0.7, 0.5), (0.35, -0.3, 0.2), (0.2, 2.0, 4.1), 0.25),
    ("parallel_misses", S.PARALLEL_BEAM, (11, 13), (9, 7, 8), (0.6, 0.7, 0.5), (0.35, -0.3, 0.2), (0.2, 2.0, 4.1), 1.0),
    ("cone_45s_grazing", S.CONE_BEAM, (16, 17), (6, 6, 6), (2.0, 2.0, 2.0), (0.0, 0.0, 0.0), (0.0, np.pi / 4, np.pi / 2), 0.5),
    # the source (5 scene units from the origin) inside the support: the gather takes the whole detector there
    ("cone_source_inside", S.CONE_BEAM, (11, 13), (7, 6, 5), (12.0, 11.0, 10.0), (0.2, 0.0, 0.1), (0.3, 2.1, 4.0), 0.5),
]


def one_hot_matrices(dev, views, det, n, s, ctr, accuracy=0.5, projection_type="interpolated"):
    """A column by column from one-hot volumes through the projector, A^T row by row from one-hot pixels through the
    back-projector: (fwd, bwd), both [rays, voxels] float32, the kernels' own bits."""
    H, W = det
    N, M = int(np.prod(n)), len(views) * H * W
    fwd = np.zeros((M, N), np.float32)
    vol = torch.zeros(N, device=dev)
    for v in range(N):
        vol.zero_()
        vol[v] = 1.0
        fwd[:, v] = K.project_views(vol.reshape(n), views, s, ctr, accuracy,
                                    projection_type=projection_type).reshape(-1).cpu().numpy()
    bwd = np.zeros((M, N), np.float32)
    pr = torch.zeros(M, device=dev)
    out = torch.empty(n, device=dev)
    for r in range(M):
        pr.zero_()
        pr[r] = 1.0
        bwd[r] = K.backproject_views(pr.reshape(len(views), H, W), views, s, ctr, accuracy, out=out,
                                     projection_type=projection_type).reshape(-1).cpu().numpy()
    return fwd, bwd


def _tiny_cfg(mode="cone", n=(6, 5, 7), det=(9, 10), sVoxel=(1.9, 1.7, 2.0), off=(0.05, -0.04, 0.03)):
    base = S.CONE_BEAM if mode == "cone" else S.PARALLEL_BEAM
    return dict(base, nVoxel=list(n), nDetector=list(det), sVoxel=list(sVoxel), offOrigin=list(off), sDetector=[3.4, 3.6],
                accuracy=0.5, filter=None)


TINY_ANGLES = np.linspace(0, 2 * np.pi, 7)[:-1] + 0.21


def tiny_system(cfg, A):
    """The right-hand side b (float32) of the tiny system: the dense matrix ``A`` of ``cfg`` at TINY_ANGLES applied to a blob
    and a disc, with 1 % multiplicative noise: a ray that only grazes the volume keeps a residual of its own size (an
    additive one would be amplified by W = 1 / (A 1) into an ill-conditioned comparison)."""
    n = tuple(cfg["nVoxel"])
    ax = [(np.arange(m) + 0.5) / m * 2 - 1 for m in n]
    X, Y, Z = np.meshgrid(*ax, indexing="ij")
    truth = (0.6 * np.exp(-(X ** 2 + Y ** 2 + Z ** 2) / 0.4) + 0.3 * ((X - 0.3) ** 2 + Y ** 2 < 0.1)).astype(np.float32)
    b = (A @ truth.ravel().astype(np.float64)).astype(np.float32)
    rng = np.random.RandomState(5)
    return (b * (1.0 + 0.01 * rng.normal(0, 1, b.shape))).astype(np.float32)
