"""Raw CT scans -> the normalised cubes that ``datagen --vol`` reads (the reference's
data_generator/synthetic_dataset/process_raw_data.py, with its resampling on the GPU: resample.py).

    python -m r2_gaussian_amd.prepare --metadata raw_metadata.py --output data_generator/volume_gt --target_size 256

The metadata is the reference's ``raw_info`` list, from a ``.py`` file that defines it (loaded as the reference loads it) or
from a ``.yml`` / ``.json`` file that holds the list (or a mapping with the key ``raw_info``).  Per case, in the reference's
order: read, normalise to [0, 1], clip, ``reshape_vol`` to ``target_size``^3, clip, transpose, inversion flags, save float32
``<output_name>.npy``; a case whose output exists is skipped.  ``file_type`` "raw" and "npy" need nothing installed; "dcm" and
"tif" need pydicom / tifffile.
"""
import argparse
import glob
import importlib.util
import json
import os
import os.path as osp

import numpy as np
import torch

from . import resample as R


def load_metadata(path):
    """-> the ``raw_info`` list of a .py, .yml / .yaml or .json metadata file."""
    ext = osp.splitext(path)[1].lower()
    if ext == ".py":
        spec = importlib.util.spec_from_file_location("metadata", path)
        module = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(module)
        return list(module.raw_info)
    if ext in (".yml", ".yaml"):
        import yaml
        with open(path) as f:
            data = yaml.safe_load(f)
    elif ext == ".json":
        with open(path) as f:
            data = json.load(f)
    else:
        raise ValueError("metadata must be a .py, .yml or .json file, got %s" % path)
    return list(data["raw_info"] if isinstance(data, dict) else data)


def _need(module, file_type):
    try:
        return importlib.import_module(module)
    except ImportError:
        raise RuntimeError("file_type %r needs the package %s, which is not installed; \"raw\" and \"npy\" need nothing"
                           % (file_type, module)) from None


def _normalise(data):
    lo, hi = data.min(), data.max()
    return (data - lo) / (hi - lo)


def _reshape(data, spacing, target_size, mode, device):
    """resample.reshape_vol for a host array, then the clip -> numpy float32."""
    vol = torch.from_numpy(np.ascontiguousarray(data, dtype=np.float32)).to(device)
    return R.reshape_vol(vol, spacing, target_size, mode).clamp_(0.0, 1.0).cpu().numpy()


def process_raw(info, target_size, device="cuda", data=None):
    """A headerless ``.raw`` file of ``dtype`` and ``shape`` (x fastest in the file), or the array ``data`` [x,y,z]."""
    if data is None:
        data = np.fromfile(info["raw_path"], dtype=info["dtype"]).reshape(info["shape"][::-1]).astype(float).transpose([2, 1, 0])
    data = _normalise(np.asarray(data, dtype=float)).clip(0.0, 1.0)
    data = _reshape(data, info["spacing"], target_size, info["reshape"], device)
    data = data.transpose(info["transpose"])
    if info["z_invert"]:
        data = data[:, :, ::-1]
    return data


def process_npy(info, target_size, device="cuda"):
    """A ``.npy`` volume [x,y,z]: the steps of a raw file."""
    return process_raw(info, target_size, device, data=np.load(info["raw_path"]))


def process_tif(info, target_size, device="cuda"):
    tifffile = _need("tifffile", "tif")
    data = _normalise(tifffile.imread(info["raw_path"]))
    data = _reshape(data, info["spacing"], target_size, info["reshape"], device)
    data = data.transpose(info["transpose"])
    if info["z_invert"]:
        data = data[:, :, ::-1]
    return data


def process_dcm(info, target_size, device="cuda"):
    pydicom = _need("pydicom", "dcm")
    slices = []
    for path in sorted(glob.glob(osp.join(info["raw_path"], "*.dcm"))):
        ds = pydicom.dcmread(path)
        slices.append(np.array(ds.pixel_array).astype(float) * float(ds.RescaleSlope) + float(ds.RescaleIntercept))
    vol = np.stack(slices, axis=-1)[:, :, ::-1]   # upside down
    vol = _normalise(vol.clip(-1000, 2000))       # from air to bone
    # the reference reads info["thickness"] and then uses the file's own SliceThickness; without a reshape mode the
    # spacing plays no part in the result either way
    spacing = np.array([float(v) for v in list(ds.PixelSpacing)] + [ds.SliceThickness])
    out = _reshape(vol, spacing, target_size, None, device)
    if info["xy_invert"]:
        out = out[::-1, ::-1, :]
    return out


PROCESSORS = {"raw": process_raw, "npy": process_npy, "tif": process_tif, "dcm": process_dcm}


def prepare(raw_info, output, target_size=256, device="cuda", verbose=True):
    """Every case of ``raw_info`` -> ``output/<output_name>.npy`` -> the list of paths (existing ones are kept)."""
    os.makedirs(output, exist_ok=True)
    paths = []
    for info in raw_info:
        path = osp.join(output, "%s.npy" % info["output_name"])
        paths.append(path)
        if osp.exists(path):
            if verbose:
                print("%s: exists, skipped" % path)
            continue
        if info["file_type"] not in PROCESSORS:
            raise ValueError("Unsupported file type")
        vol = PROCESSORS[info["file_type"]](info, target_size, device)
        np.save(path, np.ascontiguousarray(vol, dtype=np.float32))
        if verbose:
            print("%s: %s" % (path, tuple(vol.shape)))
    return paths


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--metadata", default="data_generator/raw_metadata.py", type=str, help="Path to metadata.")
    ap.add_argument("--output", default="data_generator/volume_gt", type=str, help="Path to output folder.")
    ap.add_argument("--target_size", default=256, type=int, help="Target volume size (a cube)")
    ap.add_argument("--device", default="cuda", type=str)
    args = ap.parse_args(argv)
    prepare(load_metadata(args.metadata), args.output, args.target_size, args.device)


if __name__ == "__main__":
    main()
