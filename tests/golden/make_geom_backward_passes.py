"""Records tests/golden/geom_backward_passes.npz: every gradient array of every case of tests/test_geom_backward_passes_gpu.py,
as the library that is loaded computes it on the GPU (R2HIP_LIB selects another build than the tree's, r2_gaussian_amd/_lib.py).

    python tests/golden/make_geom_backward_passes.py [out.npz]

The committed file was recorded on the commit before the geometry backward parked its moment rows as 24 bytes and was bounded to
five workgroups per CU; the test holds every later build to those bits.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from tests import test_geom_backward_passes_gpu as T   # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else T.GOLDEN
    dev = torch.device("cuda:0")
    rec = {}
    for name in T.CASES:
        rec.update(T.record_case(name, dev))
    np.savez_compressed(out, **rec)
    print("wrote %s: %d arrays, %d bytes" % (out, len(rec), os.path.getsize(out)))


if __name__ == "__main__":
    main()
