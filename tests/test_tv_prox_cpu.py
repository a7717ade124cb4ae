"""CPU: the restatement of r2_tv_prox (tests/tv_prox_ref.py) against first principles -- the closed-form solution of a 1-D
step, the identities of a proximal operator of TV -- the operator-norm bound against the singular values of a dense A, the
new entries in the header and the binding, and recon.py's host-side validation."""
import os
import re

import numpy as np
import pytest

from r2_gaussian_amd import _lib
from r2_gaussian_amd import recon as RC
from tests import recon_ref as RR
from tests import tv_prox_ref as TP
from tests.operator_cases import TINY_ANGLES, _tiny_cfg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1, 1, 40), (1, 9, 13), (2, 2, 2), (5, 1, 1), (37, 29, 53), (17, 16, 65)]


def test_entries_are_declared_and_bound():
    with open(os.path.join(ROOT, "include", "r2hip.h")) as f:
        header = f.read()
    assert re.search(r"R2_API size_t r2_tv_prox_scratch_bytes\(int nx, int ny, int nz\);", header)
    m = re.search(r"R2_API int r2_tv_prox\(([^;]*)\);", header)
    assert m
    assert len(m.group(1).split(",")) == 12 == len(_lib._SIGNATURES["r2_tv_prox"][1])
    assert len(_lib._SIGNATURES["r2_tv_prox_scratch_bytes"][1]) == 3
    syms = _lib.exported_symbols()
    assert "r2_tv_prox" in syms and "r2_tv_prox_scratch_bytes" in syms
    assert "fista_tv" in RC.METHODS and RC.METHODS[:6] == ("fdk", "sart", "ossart", "asd_pocs", "os_asd_pocs", "cgls")
    for name in ("tv_prox", "tv_denoise", "operator_norm_bound", "operator_norm_power", "fista_tv"):
        assert callable(getattr(RC, name)), name


def test_closed_form_of_a_step():
    """y = [a]*m + [b]*m with 2 lam / m <= b - a: the solution moves each plateau by lam / m towards the other."""
    m, a, b, lam = 8, 0.2, 0.9, 0.5
    assert 2 * lam / m <= b - a
    y = np.array([a] * m + [b] * m).reshape(1, 1, 2 * m)
    want = np.array([a + lam / m] * m + [b - lam / m] * m).reshape(1, 1, 2 * m)
    e200 = float(np.abs(TP.tv_prox64(y, lam, 200) - want).max())
    e1000 = float(np.abs(TP.tv_prox64(y, lam, 1000) - want).max())
    print("closed form: max error %.3g at 200 iterations, %.3g at 1000" % (e200, e1000))
    assert e200 < 1e-4, e200
    assert e1000 < e200, (e1000, e200)
    # the float32 restatement reaches the same point within its precision
    assert float(np.abs(TP.tv_prox32(y, lam, 200).astype(np.float64) - want).max()) < 1e-4 + 1e-5


@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_identities_of_the_restatement(shape):
    rng = np.random.RandomState(sum(shape))
    y = rng.rand(*shape)
    c = np.full(shape, 0.3)
    assert np.array_equal(TP.tv_prox64(c, 0.5, 30), c)
    assert np.array_equal(TP.tv_prox32(c, 0.5, 30), c.astype(np.float32))
    assert np.array_equal(TP.tv_prox64(y - 0.5, 0.0, 30, lo=0.0, hi=0.25), np.clip(y - 0.5, 0.0, 0.25))
    assert np.array_equal(TP.tv_prox64(y, -1.0, 30), y) and np.array_equal(TP.tv_prox64(y, float("nan"), 30), y)
    assert np.array_equal(TP.tv_prox64(y - 0.5, 0.3, 0, lo=0.0), np.maximum(y - 0.5, 0.0))
    for lam in (0.05, 0.5):
        x = TP.tv_prox64(y, lam, 30)
        assert abs(x.mean() - y.mean()) < 1e-12, (lam, x.mean() - y.mean())   # sum D^T p = 0
        assert TP.tv_value(x) < TP.tv_value(y), lam
        assert TP.objective(x, y, lam) < TP.objective(y, y, lam), lam
        xb = TP.tv_prox64(y - 0.5, lam, 30, lo=0.0)
        assert xb.min() >= 0.0
        x32 = TP.tv_prox32(y.astype(np.float32), lam, 30)
        assert x32.dtype == np.float32
        # the float32 run follows the float64 one: 30 iterations of about 20 operations each on values of order one, one
        # rounding of 2^-24 per operation, added up linearly
        assert float(np.abs(x32 - TP.tv_prox64(y.astype(np.float32), lam, 30)).max()) < 30 * 20 * 2.0 ** -24


def test_operator_norm_bound_dominates_the_largest_singular_value():
    for mode in ("cone", "parallel"):
        A, _ = RR.dense_A_cfg(_tiny_cfg(mode), TINY_ANGLES)
        assert (A >= 0).all()   # what makes |A|_2^2 <= |A|_1 |A|_inf usable as max(A 1) max(A^T 1)
        s = np.linalg.svd(A, compute_uv=False)[0]
        bound = TP.operator_norm_bound(A)
        print("|A|_2^2 = %.6g, bound = %.6g (%s)" % (s * s, bound, mode))
        assert bound >= s * s


def test_fista_restatement_decreases_its_objective():
    cfg = _tiny_cfg("cone")
    A, _ = RR.dense_A_cfg(cfg, TINY_ANGLES)
    from tests.operator_cases import tiny_system
    b = tiny_system(cfg, A).astype(np.float64)
    n = tuple(cfg["nVoxel"])
    xs, lam, L = TP.fista_tv(A, b, n, 30, 1e-2, 50)
    f = [TP.fista_objective(A, b, x, lam, n) for x in xs]
    assert f[-1] < TP.fista_objective(A, b, np.zeros(A.shape[1]), lam, n)
    assert f[-1] < f[0] and min(x.min() for x in xs) >= 0.0


def test_host_side_validation():
    import torch
    with pytest.raises(_lib.R2HipError):
        RC.tv_prox(torch.zeros(3, 3, 3), 0.1, 1)
    with pytest.raises(NotImplementedError):
        RC.reconstruct(np.zeros((1, 9, 10), np.float32), [0.0], _tiny_cfg(), "fista")
