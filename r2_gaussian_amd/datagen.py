"""Synthetic CT dataset generation without TIGRE: ``main`` of data_generator/synthetic_dataset/generate_data.py on the
projector of projector.py.

    python -m r2_gaussian_amd.datagen --vol vol.npy --scanner cone_beam.yml --output data/case_dir [--n_train 50]
                                      [--n_test 100] [--seed 0] [--projection_type interpolated|siddon]
                                      [--stripes N AMPLITUDE]

writes ``{output}/{vol_name}_{mode}/`` with ``vol_gt.npy``, ``proj_train/proj_train_%04d.npy``,
``proj_test/proj_test_%04d.npy`` (float32 [H, W], the rasterizer's row order) and ``meta_data.json`` (keys scanner, vol,
bbox, proj_train, proj_test; each projection entry {file_path, angle}) -- the layout dataset_readers.py reads.

Training angles are linspace(0, totalAngle, n_train + 1)[:-1] + startAngle, test angles sort(rand(n_test) 2 pi) + startAngle
(radians; the config's angles are degrees).  With ``noise: true`` the training stack gets ``add_noise`` (TIGRE's
``CTnoise.add``) and its negatives are clipped to 0; test projections stay noise-free.  Every draw comes from one explicit
``numpy.random.RandomState`` (``--seed``), so a seed reproduces a dataset bit for bit -- the reference draws from numpy's
global generator.  ``--projection_type siddon`` projects with the ray-voxel intersection model instead of the interpolated
one; a case made with a model named explicitly records it as ``projection_type`` in its saved scanner config.

``--dead_pixels F``, ``--dead_lines N``, ``--gap C0 C1`` (none by default) draw one static detector mask (``weights.defect_mask``,
after every other draw): the masked pixels of the TRAINING projections are written as 0, the mask as ``weights_train.npy``
([H, W] float32, 1 = measured) and under the key ``weights_train`` of ``meta_data.json``.  Without them a case is, byte for
byte, what it was.
"""
import argparse
import json
import os
import os.path as osp

import numpy as np

from . import projector as P


def add_noise(projs, i0, gaussian, rng):
    """Restatement of TIGRE's ``CTnoise.add(projs, Poisson=i0, Gaussian=[mu, sigma])`` applied to the whole stack,
    followed by the clip of negatives of generate_data.py:59: with m = max(projs),
    I = Poisson(i0 exp(-projs / m)) + Normal(mu, sigma), I <= 0 -> 1e-6, projs = -log(I / i0) m, then max(projs, 0).
    Unpinned: TIGRE is not available to compare against, this follows its published source.  Draws: first the Poisson
    field, then the normal field, both from ``rng`` (a numpy RandomState) in C order.  float32 result."""
    p = np.asarray(projs, dtype=np.float64)
    mu, sigma = (float(x) for x in gaussian)
    m = float(p.max())
    if not m > 0:
        return np.asarray(projs, dtype=np.float32).copy()   # an all-zero stack: exp(-0/0) is undefined, nothing attenuates
    intensity = rng.poisson(i0 * np.exp(-p / m)).astype(np.float64)
    intensity = intensity + rng.normal(mu, sigma, size=p.shape)
    intensity[intensity <= 0] = 1e-6
    out = (-np.log(intensity / i0) * m).astype(np.float32)
    out[out < 0.0] = 0.0
    return out


def noisy_train(projs, cfg, rng):
    """The training stack as generate_data.py:51-60 saves it: ``add_noise`` when the config says ``noise: true``, else
    ``projs`` itself."""
    if not cfg.get("noise", False):
        return projs
    return add_noise(projs, cfg["possion_noise"], cfg["gaussian_noise"], rng)


def angles_for(cfg, n_train, n_test, rng):
    """-> (train angles, test angles) in radians (generate_data.py:47-50, 63-66)."""
    start = cfg.get("startAngle", 0.0) / 180.0 * np.pi
    train = np.linspace(0.0, cfg.get("totalAngle", 360.0) / 180.0 * np.pi, n_train + 1)[:-1] + start
    test = np.sort(rng.rand(n_test) * 360.0 / 180.0 * np.pi) + start
    return train, test


STRIPE_STREAM = 0x57121E5   # the second seed word of the stripes' own generator


def stripe_field(nDetector, n, amplitude, seed):
    """The static offsets of ``n`` miscalibrated detector columns for ``nDetector`` = (H, W) -> (columns, field): the sorted
    list of the n distinct columns and the float32 [H, W] field that every view gains, N(0, amplitude) per (row, column) of
    those columns and 0 elsewhere.  Deterministic in ``seed`` through a RandomState of its own: first the columns, then the
    offsets in C order."""
    H, W = int(nDetector[0]), int(nDetector[1])
    if int(n) != n or not 0 <= int(n) <= W:
        raise ValueError("stripes must be an integer number of columns in [0, %d], got %r" % (W, n))
    if not float(amplitude) >= 0.0:
        raise ValueError("the stripes' amplitude must be >= 0, got %r" % (amplitude,))
    rng = np.random.RandomState([int(seed) % 2 ** 32, STRIPE_STREAM])
    columns = np.sort(rng.choice(W, size=int(n), replace=False))
    field = np.zeros((H, W), np.float32)
    field[:, columns] = rng.normal(0.0, float(amplitude), size=(H, int(n))).astype(np.float32)
    return [int(c) for c in columns], field


def write_case(case_dir, cfg, vol, projs_train, angles_train, projs_test, angles_test, weights_train=None, stripe_columns=None):
    """The on-disk layout of generate_data.py:70-100 for given projections [V, H, W]; -> the meta dictionary written.
    ``weights_train`` ([H, W], shared by the training views, or [V, H, W]; None: the case records none and is the
    reference's layout): saved as ``weights_train.npy`` and recorded under the key ``weights_train``.  ``stripe_columns``: None,
    or the list of miscalibrated detector columns to record under the key ``stripe_columns``."""
    os.makedirs(case_dir, exist_ok=True)
    np.save(osp.join(case_dir, "vol_gt.npy"), np.asarray(vol, dtype=np.float32))
    entries = {}
    for split, projs, angles in (("proj_train", projs_train, angles_train), ("proj_test", projs_test, angles_test)):
        os.makedirs(osp.join(case_dir, split), exist_ok=True)
        entries[split] = []
        for i in range(len(angles)):
            name = osp.join(split, "%s_%04d.npy" % (split, i))
            np.save(osp.join(case_dir, name), np.ascontiguousarray(projs[i], dtype=np.float32))
            entries[split].append({"file_path": name, "angle": float(angles[i])})
    meta = {"scanner": cfg, "vol": "vol_gt.npy", "bbox": [[-1, -1, -1], [1, 1, 1]],
            "proj_train": entries["proj_train"], "proj_test": entries["proj_test"]}
    if weights_train is not None:
        w = np.ascontiguousarray(weights_train, dtype=np.float32)
        if w.shape != np.shape(projs_train)[-2:] and w.shape != np.shape(projs_train):
            raise ValueError("weights_train is %s but the training projections are %s" % (w.shape, np.shape(projs_train)))
        np.save(osp.join(case_dir, "weights_train.npy"), w)
        meta["weights_train"] = "weights_train.npy"
    if stripe_columns is not None:
        meta["stripe_columns"] = [int(c) for c in stripe_columns]
    with open(osp.join(case_dir, "meta_data.json"), "w", encoding="utf-8") as f:
        json.dump(meta, f, indent=4)
    return meta


def recorded_projection_type(cfg):
    """The projector model a saved scanner config records ("interpolated" for a case that records none)."""
    return P.check_projection_type(cfg.get("projection_type", "interpolated"))


def generate(vol, cfg, output, vol_name, n_train=50, n_test=100, seed=0, device="cuda", projection_type=None, defects=None,
             stripes=None):
    """Project ``vol`` [nx,ny,nz] with the raw scanner config ``cfg`` and write the case ``{output}/{vol_name}_{mode}``;
    -> the case directory.  ``projection_type``: "interpolated" or "siddon", written into the case's saved scanner config;
    None takes the config's own ``projection_type`` ("interpolated" if absent) and saves the config as it is.
    ``defects``: None, or the keyword arguments of ``weights.defect_mask`` (dead_pixels, dead_lines, gap) for one static
    detector mask, drawn after every other draw: the training projections are written with 0 in the masked pixels and the mask
    as the case's ``weights_train``.  ``stripes``: None, or (n, amplitude) for ``stripe_field``: its field is added to every
    training view (after the noise, before the mask) and every test view."""
    if projection_type is None:
        projection_type = recorded_projection_type(cfg)
    else:
        cfg = dict(cfg, projection_type=P.check_projection_type(projection_type))
    rng = np.random.RandomState(seed)
    vol = np.asarray(vol, dtype=np.float32)
    train_angles, test_angles = angles_for(cfg, n_train, n_test, rng)
    train = P.project(vol, train_angles, cfg, device=device, projection_type=projection_type).cpu().numpy()
    train = noisy_train(train, cfg, rng)
    test = P.project(vol, test_angles, cfg, device=device, projection_type=projection_type).cpu().numpy()
    case_dir = osp.join(output, "%s_%s" % (vol_name, cfg["mode"]))
    columns = None
    if stripes is not None:
        columns, field = stripe_field(cfg["nDetector"], stripes[0], stripes[1], seed)
        train, test = (train + field[None]).astype(np.float32), (test + field[None]).astype(np.float32)
    mask = None
    if defects:
        from .weights import defect_mask
        mask = defect_mask(cfg["nDetector"], rng, **defects)
        train = np.where(mask > 0, train, np.float32(0)).astype(np.float32)
    write_case(case_dir, cfg, vol, train, train_angles, test, test_angles, weights_train=mask, stripe_columns=columns)
    return case_dir


def main(argv=None):
    ap = argparse.ArgumentParser(description="Data generator parameters")
    ap.add_argument("--vol", default="data_generator/volume_gt/0_chest.npy", type=str, help="Path to volume.")
    ap.add_argument("--scanner", default="data_generator/scanner/cone_beam.yml", type=str,
                    help="Path to scanner configuration.")
    ap.add_argument("--output", default="data/cone_ntrain_50_angle_360", type=str, help="Path to output.")
    ap.add_argument("--n_train", default=50, type=int, help="Number of projections for training.")
    ap.add_argument("--n_test", default=100, type=int, help="Number of projections for evaluation.")
    ap.add_argument("--seed", default=0, type=int, help="Seed of every random draw (test angles, noise).")
    ap.add_argument("--projection_type", default=None, choices=P.PROJECTION_TYPES,
                    help="Projector model (default: the scanner configuration's, else interpolated).")
    ap.add_argument("--dead_pixels", default=0.0, type=float, help="Fraction of singly dead detector pixels.")
    ap.add_argument("--dead_lines", default=0, type=int, help="Number of dead detector rows or columns.")
    ap.add_argument("--gap", default=None, type=int, nargs=2, metavar=("C0", "C1"),
                    help="A band of unmeasured detector columns C0 <= c < C1.")
    ap.add_argument("--stripes", default=None, nargs=2, metavar=("N", "AMPLITUDE"),
                    help="N miscalibrated detector columns with offsets drawn from N(0, AMPLITUDE), the same in every view.")
    args = ap.parse_args(argv)
    stripes = None
    if args.stripes is not None:
        try:
            stripes = (int(args.stripes[0]), float(args.stripes[1]))
        except ValueError:
            ap.error("--stripes takes an integer N and a number AMPLITUDE, got %r" % (args.stripes,))
    import yaml
    with open(args.scanner, "r") as f:
        cfg = yaml.safe_load(f)
    vol_name = osp.basename(args.vol)[:-4]
    print("Generate data for case %s_%s" % (vol_name, cfg["mode"]))
    defects = None
    if args.dead_pixels > 0 or args.dead_lines > 0 or args.gap is not None:
        defects = dict(dead_pixels=args.dead_pixels, dead_lines=args.dead_lines, gap=None if args.gap is None else tuple(args.gap))
    case_dir = generate(np.load(args.vol), cfg, args.output, vol_name, args.n_train, args.n_test, args.seed,
                        projection_type=args.projection_type, defects=defects, stripes=stripes)
    print("Generate data for case %s complete!" % osp.basename(case_dir))
    return case_dir


if __name__ == "__main__":
    main()
