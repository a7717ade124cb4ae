"""CPU: the arithmetic half of csrc/cloud_model.hpp -- the one statement of the activations and of the quaternion's rotation
matrix that gaussian_step.hip, densify_ops.hip, gaussian_mcmc.hip and gaussian_merge.hip share -- built by plain g++
(tests/cloud_model_main.cpp) and compared bit for bit with a numpy restatement in the same operation order."""
import os
import shutil
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def quat_rot(q):
    """cloud_model.hpp's quat_rot on rows (r, x, y, z) of q, in q's dtype: only + - *, each rounded once, so IEEE arithmetic
    gives the header's bits.  -> [n, 9], the rows of R one after the other."""
    r, x, y, z = (q[:, k] for k in range(4))
    one, two = q.dtype.type(1), q.dtype.type(2)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        R = [one - two * (y * y + z * z), two * (x * y - r * z), two * (x * z + r * y),
             two * (x * y + r * z), one - two * (x * x + z * z), two * (y * z - r * x),
             two * (x * z - r * y), two * (y * z + r * x), one - two * (x * x + y * y)]
    return np.stack(R, axis=1)


def quaternions(dtype, seed):
    """300 rows: the edge cases first (all zero, unnormalised, denormal components, components near 1e19 whose products overflow
    float32), then normalised, unnormalised and widely scaled random ones."""
    g = np.random.RandomState(seed)
    tiny = np.finfo(dtype).tiny
    edge = np.array([[0, 0, 0, 0], [3, -4, 12, 0.5], [tiny / 4, -tiny / 8, tiny / 2, tiny / 16], [1, tiny / 4, 0, -tiny / 2],
                     [1e19, -1.5e19, 1.2e19, 0.9e19], [2e19, 2e19, 2e19, -2e19], [-0.0, 0.0, -0.0, 1.0]], dtype=np.float64)
    unit = g.standard_normal((100, 4))
    unit /= np.linalg.norm(unit, axis=1, keepdims=True)
    loose = g.standard_normal((100, 4)) * 3
    wide = g.standard_normal((300 - 200 - len(edge), 4)) * 10.0 ** g.uniform(-30, 18, (300 - 200 - len(edge), 1))
    return np.concatenate([edge, unit, loose, wide]).astype(dtype)


def test_the_header_on_the_host(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++"))
    assert cxx, "no C++ compiler"
    exe = str(tmp_path / "cloud_model_main")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-ffp-contract=off", "-fsanitize=undefined", "-static-libubsan",
                        "-fno-sanitize-recover=all", "-Wall", "-Werror", os.path.join(HERE, "cloud_model_main.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    q32, q64 = quaternions(np.float32, 1), quaternions(np.float64, 2)
    assert (np.abs(q32[2]) < np.finfo(np.float32).tiny).all() and (q32[2] != 0).all()     # the denormals stayed denormal
    acts = np.array([20.0, np.nextafter(np.float32(20), np.float32(21)), 20.5, 25.0, 88.0, 1e10, 3e38, np.inf,   # > 20, but the first
                     -100.0, -1.0, 0.0, 0.5, 19.999, -np.inf], np.float32)
    lines = ["f " + " ".join(float(v).hex() for v in row) for row in q32]
    lines += ["d " + " ".join(float(v).hex() for v in row) for row in q64]
    lines += ["a " + float(v).hex() for v in acts]
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "cloud model ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    out = [ln.split() for ln in r.stdout.splitlines()]
    got32 = np.array([[int(x, 16) for x in ln[1:]] for ln in out if ln[0] == "f"], np.uint32)
    got64 = np.array([[int(x, 16) for x in ln[1:]] for ln in out if ln[0] == "d"], np.uint64)
    assert got32.shape == (300, 9) and got64.shape == (300, 9)
    assert (got32 == quat_rot(q32).view(np.uint32)).all()
    assert (got64 == quat_rot(q64).view(np.uint64)).all()
    assert np.isnan(quat_rot(q32)[5]).any() and np.isfinite(quat_rot(q64)[5]).all()        # inf - inf in float32 only
    # the branch identities: past the threshold the softplus and the rounded inverse return their argument's bits, and
    # without a bound the scale activation is expf whatever range and lo say
    rows = np.array([[int(x, 16) for x in ln[1:]] for ln in out if ln[0] == "a"], np.uint32)
    assert (rows[:, 0] == acts.view(np.uint32)).all()
    above = acts > 20
    assert above.sum() == 7 and (rows[above, 1] == rows[above, 0]).all() and (rows[above, 2] == rows[above, 0]).all()
    assert (rows[:, 3] == rows[:, 4]).all()
