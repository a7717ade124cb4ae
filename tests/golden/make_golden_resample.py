"""Writes tests/golden/resample/*.npz: scipy.ndimage's own float64 results for the cases of tests/resample_ref.py, so that no
test needs scipy at run time.  Needs scipy (written with 1.15).

    python -m tests.golden.make_golden_resample
"""
import os

import numpy as np
import scipy.ndimage as ndimage

from tests import resample_ref as R

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "resample")


def scipy_zoom(vol, factor):
    return ndimage.zoom(np.asarray(vol, dtype=np.float64), factor, mode="nearest")


def main():
    os.makedirs(OUT, exist_ok=True)
    for shape, factors in R.ZOOM_CASES:
        vol = R.case_volume(shape)
        data = {"vol": vol}
        for f in factors:
            data["zoom_" + R.factor_id(f)] = scipy_zoom(vol, f)
        np.savez(os.path.join(OUT, "zoom_%s.npz" % "x".join(map(str, shape))), **data)
    for shape in R.SAMPLE_SHAPES:
        vol, pts = R.case_volume(shape), R.case_points(shape)
        want = ndimage.map_coordinates(vol.astype(np.float64), pts.astype(np.float64).T, order=3, mode="nearest")
        np.savez(os.path.join(OUT, "sample_%s.npz" % "x".join(map(str, shape))), vol=vol, points=pts, values=want)
    for shape, spacing, target, mode in R.RESHAPE_CASES:
        vol = R.case_volume(shape)
        want = R.reshape_vol(vol.astype(np.float64), spacing, target, mode, zoom_fn=scipy_zoom)
        np.savez(os.path.join(OUT, "reshape_%s.npz" % mode), vol=vol, spacing=np.array(spacing), target=target, out=want)


if __name__ == "__main__":
    main()
