"""Measured cone-beam scans -> a case that ``train`` and ``recon`` read (the reference's
data_generator/real_dataset/generate_data.py, with its cv2 / numpy conditioning on the GPU: projections.py, and fdk.py in
TIGRE's place).

    python -m r2_gaussian_amd.prepare_real --data fips/pine --output data/real/pine [--proj_subsample 4]
                                           [--interpolation {linear,area}] [--despeckle THRESH [--despeckle_size K]]
                                           [--destripe K [--destripe_method {sort,mean}]]

``--data`` holds the FIPS ``config.txt`` and one projection per file: ``*.mat`` with the variable ``img`` (read with
``scipy.io.loadmat``), or ``*.npy`` when there is no ``.mat``.  Per projection, in the reference's order:
``/ proj_rescale * object_scale`` and the float32 cast on the host; then on the device values below 0 become 0, the image moves
up by five rows (the dataset's description; zeros come in below), and with ``--proj_subsample`` other than 1 it is resized to
``int(h / s) x int(w / s)`` and cropped to the reference's centred square.  ``--despeckle THRESH`` first replaces, at full
resolution, every pixel further than THRESH from the median of its K x K window (and every NaN) by that median.
``--destripe K`` removes the stripes of miscalibrated detector pixels, the rings of the reconstruction
(``projections.destripe``, a median across K detector columns): that needs all views of a detector row at once, so it runs on
the whole conditioned stack -- after the resize, through which a gain error survives as the mean over the merged pixels, and
before anything is written -- in bands of detector rows where the stack is larger than the device.  The
projections go to ``proj_all/``, the reference's choice of training and test views also to ``proj_train/`` and ``proj_test/``,
``vol_gt.npy`` is the FDK reconstruction of all of them clamped at 0 (kept when it exists), and ``meta_data.json`` holds the
reference's scanner block.

Against the reference: the resize follows cv2's sampling rule and weights in a stated float32 order, not cv2's own bits;
``meta_data.json`` names the volume under ``"vol"``, which the readers read, next to the reference's ``"ct"``; and a side
difference of 1 after the resize, where the reference's ``[0:-0]`` slice silently gives an empty image, raises.
"""
import argparse
import glob
import json
import os
import os.path as osp
import random

import numpy as np
import torch

from . import fdk as F
from . import projections as PJ

ROW_SHIFT = 5   # rows the FIPS detector images are moved up by, as the data sets' description asks


# config.txt: (text that names the key, name here, type), tried in this order on every line
_CONFIG_KEYS = (("NumberImages", "n_proj", int), ("AngleInterval", "angle_interval", float), ("AngleFirst", "angle_start", float),
                ("AngleLast", "angle_last", float), ("DistanceSourceDetector", "DSD_mm", float),
                ("DistanceSourceOrigin", "DSO_mm", float), ("PixelSize", "pixel_mm", float))


def parse_config(path, proj_subsample, object_scale):
    """FIPS ``config.txt`` by the reference's rule: a line belongs to the first key whose text it contains, its value is what
    follows its last ``=``, a later line overrides an earlier one, and ``PixelSizeUnit`` is no ``PixelSize``.  Lengths are
    millimetres in the file.  -> dict n_proj, angle_interval, angle_start, angle_last (degrees), DSD, DSO and dDetector (the
    pixel pitch after the subsampling), the lengths in metres times ``object_scale``."""
    raw = {}
    with open(path, "r") as f:
        for line in f:
            for text, name, kind in _CONFIG_KEYS:
                if text in line:
                    if not (text == "PixelSize" and "PixelSizeUnit" in line):
                        raw[name] = kind(line.split("=")[-1])
                    break
    missing = [text for text, name, _ in _CONFIG_KEYS if name not in raw]
    if missing:
        raise ValueError("%s does not give %s" % (path, ", ".join(missing)))
    c = {k: raw[k] for k in ("n_proj", "angle_interval", "angle_start", "angle_last")}
    c["DSD"] = raw["DSD_mm"] / 1000 * object_scale
    c["DSO"] = raw["DSO_mm"] / 1000 * object_scale
    c["dDetector"] = raw["pixel_mm"] * proj_subsample / 1000 * object_scale
    return c


def scan_angles(cfg):
    """Every projection's angle in radians."""
    angles = np.concatenate([np.arange(cfg["angle_start"], cfg["angle_last"], cfg["angle_interval"]), [cfg["angle_last"]]])
    return angles / 180.0 * np.pi


def select_ids(n_proj, n_train, n_test):
    """The reference's training and test views: evenly spaced ones, and a sample of the rest drawn as ``random.seed(0);
    random.sample`` draws it (a generator of its own with that seed: the same numbers, the caller's generator untouched)."""
    train_ids = np.linspace(0, n_proj - 1, n_train).astype(int)
    test_ids = sorted(random.Random(0).sample(np.setdiff1d(np.arange(n_proj), train_ids).tolist(), n_test))
    return train_ids, test_ids


def crop_window(mh, mw):
    """The reference's square crop of a resized mh x mw image as (r0, c0, oh, ow): ``proj[off:-off]`` along the longer side
    with ``off = int(difference / 2)``, so an odd difference leaves one row or column more than a square."""
    if mh == mw:
        return 0, 0, mh, mw
    off = int(abs(mh - mw) / 2)
    if off == 0:
        raise ValueError("resized projections of %d x %d differ by one between their sides: the reference's crop [0:-0] is "
                         "empty there; choose another --proj_subsample" % (mh, mw))
    return (off, 0, mh - 2 * off, mw) if mh > mw else (0, off, mh, mw - 2 * off)


def resized_size(h, w, proj_subsample):
    return int(h / proj_subsample), int(w / proj_subsample)


def load_projection(path, proj_rescale, object_scale):
    """One measured projection, scaled and cast as the reference does on the host -> float32 [H,W]."""
    if path.endswith(".mat"):
        try:
            import scipy.io
        except ImportError:
            raise RuntimeError("reading %s needs scipy (scipy.io.loadmat), which is not installed; "
                               "projections saved as .npy need nothing" % path) from None
        img = scipy.io.loadmat(path)["img"]
    else:
        img = np.load(path)
    proj = img / proj_rescale * object_scale
    return proj.astype(np.float32)


def condition(projs, proj_subsample=4, interpolation="linear", despeckle=None, despeckle_size=3):
    """The device part: [V,H,W] float32 on the GPU -> the conditioned stack (despeckle, clamp at 0, row shift, resize, crop)."""
    if despeckle is not None:
        projs = PJ.despeckle(projs, despeckle, size=despeckle_size)
    H, W = projs.shape[-2:]
    if proj_subsample == 1.0:
        out = torch.zeros_like(projs, dtype=torch.float32)
        n = max(H - ROW_SHIFT, 0)
        out[..., :n, :] = projs[..., ROW_SHIFT:ROW_SHIFT + n, :]
        return torch.where(out < 0, torch.zeros_like(out), out)
    mh, mw = resized_size(H, W, proj_subsample)
    return PJ.resize(projs, (mh, mw), interpolation, shift=(ROW_SHIFT, 0), lo=0.0, crop=crop_window(mh, mw))


def destripe_rows(stack, size, method="sort", device="cuda", rows=None):
    """``projections.destripe`` of a host stack [V,H,W] (float32) -> a new host stack.  Stripe removal needs all views of a
    detector row at once but rows are independent, so the stack visits the device in bands of ``rows`` detector rows: by default
    as many as fit in four fifths of the device's free memory (a band, its result and the sort method's workspace are 14 bytes
    per value)."""
    V, H, W = stack.shape
    if rows is None:
        free = torch.cuda.mem_get_info(torch.device(device))[0]
        rows = int(free * 4 // 5 // max(14 * V * W, 1))
        if rows < 1:
            raise ValueError("one detector row of %d views x %d columns does not fit on the device" % (V, W))
    out = np.empty(stack.shape, dtype=np.float32)
    for h0 in range(0, H, rows):
        band = torch.from_numpy(np.ascontiguousarray(stack[:, h0:h0 + rows], dtype=np.float32)).to(device)
        out[:, h0:h0 + rows] = PJ.destripe(band, size, method).cpu().numpy()
    return out


def projection_paths(data):
    paths = sorted(glob.glob(osp.join(data, "*.mat")))
    return paths if paths else sorted(glob.glob(osp.join(data, "*.npy")))


def convert(args, device="cuda"):
    """generate_data.py:main for the parsed arguments -> the meta dictionary written."""
    cfg = parse_config(osp.join(args.data, "config.txt"), args.proj_subsample, args.object_scale)
    angles = scan_angles(cfg)
    output_path = args.output
    all_save_path = osp.join(output_path, "proj_all")
    train_save_path = osp.join(output_path, "proj_train")
    test_save_path = osp.join(output_path, "proj_test")
    for p in (all_save_path, train_save_path, test_save_path):
        os.makedirs(p, exist_ok=True)
    paths = projection_paths(args.data)
    if not paths:
        raise ValueError("no *.mat or *.npy projections in %s" % args.data)
    train_ids, test_ids = select_ids(cfg["n_proj"], args.n_train, args.n_test)
    projection_train_list, projection_test_list = [], []

    def save(i_proj, path, image):
        name = osp.basename(path).split(".")[0] + ".npy"
        np.save(osp.join(all_save_path, name), image)
        if i_proj in train_ids:
            np.save(osp.join(train_save_path, name), image)
            projection_train_list.append({"file_path": osp.join(osp.basename(train_save_path), name), "angle": float(angles[i_proj])})
        elif i_proj in test_ids:
            np.save(osp.join(test_save_path, name), image)
            projection_test_list.append({"file_path": osp.join(osp.basename(test_save_path), name), "angle": float(angles[i_proj])})

    conditioned = []   # with --destripe: the conditioned stack, which is written only once all of its views are known
    # a few projections at a time: a full-resolution stack is larger than the device
    for i0 in range(0, len(paths), args.batch):
        batch = paths[i0:i0 + args.batch]
        host = np.stack([load_projection(p, args.proj_rescale, args.object_scale) for p in batch])
        out = condition(torch.from_numpy(host).to(device), args.proj_subsample, args.interpolation, args.despeckle,
                        args.despeckle_size).cpu().numpy()
        if args.destripe is not None:
            conditioned.append(out)
            continue
        for k, path in enumerate(batch):
            save(i0 + k, path, out[k])
    if args.destripe is not None:
        stack = destripe_rows(np.concatenate(conditioned), args.destripe, args.destripe_method, device)
        for i_proj, path in enumerate(paths):
            save(i_proj, path, stack[i_proj])
    if not projection_train_list:
        raise ValueError("no training projection among the %d files of %s" % (len(paths), args.data))

    proj = np.load(osp.join(output_path, projection_train_list[0]["file_path"]))
    nDetector = [proj.shape[0], proj.shape[1]]
    sDetector = np.array(nDetector) * np.array(cfg["dDetector"])
    offOrigin, sVoxel = args.offOrigin, args.sVoxel
    bbox = np.array([np.array(offOrigin) - np.array(sVoxel) / 2, np.array(offOrigin) + np.array(sVoxel) / 2]).tolist()
    scanner_cfg = {
        "mode": "cone",
        "DSD": cfg["DSD"],
        "DSO": cfg["DSO"],
        "nDetector": nDetector,
        "sDetector": sDetector.tolist(),
        "nVoxel": args.nVoxel,
        "sVoxel": sVoxel,
        "offOrigin": offOrigin,
        "offDetector": args.offDetector,
        "accuracy": args.accuracy,
        "totalAngle": cfg["angle_last"] - cfg["angle_start"],
        "startAngle": cfg["angle_start"],
        "noise": True,
        "filter": None,
    }

    ct_gt_save_path = osp.join(output_path, "vol_gt.npy")
    if not osp.exists(ct_gt_save_path):
        proj_paths = sorted(glob.glob(osp.join(all_save_path, "*.npy")))
        if len(proj_paths) != len(angles):
            raise ValueError("%d projections in %s but config.txt describes %d angles" % (len(proj_paths), all_save_path, len(angles)))
        projs = np.stack([np.load(p) for p in proj_paths], axis=0)
        print("reconstruct with FDK")
        ct_gt = F.fdk(projs, angles, scanner_cfg, device=device).clamp_min_(0.0)
        np.save(ct_gt_save_path, ct_gt.cpu().numpy())

    meta_data = {
        "scanner": scanner_cfg,
        "ct": "vol_gt.npy",
        "vol": "vol_gt.npy",
        "radius": 1.0,
        "bbox": bbox,
        "proj_train": projection_train_list,
        "proj_test": projection_test_list,
    }
    with open(osp.join(output_path, "meta_data.json"), "w", encoding="utf-8") as f:
        json.dump(meta_data, f, indent=4)
    print("Data saved in %s" % output_path)
    return meta_data


def parser():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--data", type=str, help="Folder with config.txt and the measured projections.")
    ap.add_argument("--output", type=str, help="Folder of the case to write.")
    ap.add_argument("--proj_subsample", default=4, type=int, help="Factor by which the detector is down-sampled.")
    ap.add_argument("--proj_rescale", default=400.0, type=float, help="Projection values are divided by this (densities near [0, 1]).")
    ap.add_argument("--object_scale", default=50, type=int, help="Scale of the scene, to the size of the synthetic cases.")
    ap.add_argument("--n_test", default=100, type=int, help="Number of test views.")
    ap.add_argument("--n_train", default=75, type=int, help="Number of training views.")
    ap.add_argument("--nVoxel", nargs="+", default=[256, 256, 256], type=int, help="Voxels of the volume.")
    ap.add_argument("--sVoxel", nargs="+", default=[2.0, 2.0, 2.0], type=float, help="Size of the volume.")
    ap.add_argument("--offOrigin", nargs="+", default=[0.0, 0.0, 0.0], type=float, help="Offset of the volume's centre.")
    ap.add_argument("--offDetector", nargs="+", default=[0.0, 0.0], type=float, help="Offset of the detector.")
    ap.add_argument("--accuracy", default=0.5, type=float, help="Recorded in the scanner block (a TIGRE setting).")
    ap.add_argument("--interpolation", default="linear", choices=sorted(PJ.INTERPOLATIONS),
                    help="Resize rule: linear is the reference's cv2.resize, area the box mean (integer factors).")
    ap.add_argument("--despeckle", default=None, type=float, metavar="THRESH",
                    help="Replace pixels further than THRESH from their window's median, at full resolution (off by default).")
    ap.add_argument("--despeckle_size", default=3, type=int, choices=(3, 5), help="Side of the despeckle window.")
    ap.add_argument("--destripe", default=None, type=int, metavar="K",
                    help="Remove stripes (rings) from the conditioned stack with a median of K detector columns (off by default).")
    ap.add_argument("--destripe_method", default="sort", choices=sorted(PJ.DESTRIPE_METHODS),
                    help="sort: sorting-based (Vo et al. 2018), also partial stripes; mean: the mean profile, full stripes only.")
    ap.add_argument("--batch", default=8, type=int, help="Projections on the device at a time.")
    ap.add_argument("--device", default="cuda", type=str)
    return ap


def main(argv=None):
    args = parser().parse_args(argv)
    if args.data is None or args.output is None:
        raise SystemExit("--data and --output are required")
    if args.batch < 1:
        raise SystemExit("--batch must be at least 1")
    if args.destripe is not None and (args.destripe % 2 != 1 or not 1 <= args.destripe <= 31):
        raise SystemExit("--destripe takes an odd window width in 1 .. 31")
    return convert(args, args.device)


if __name__ == "__main__":
    main()
