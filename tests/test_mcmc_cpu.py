"""CPU: the restatement of the relocation / position-noise contract (tests/mcmc_ref.py): the generator's published known
answers, in numpy and in csrc/philox.hpp built by plain g++ (tests/philox_main.cpp); the measured float32 errors the GPU
tolerances are taken from; the statistics of the integer sampler and of the normals; the trainer's new flags."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import mcmc_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))


def test_known_answers():
    """Random123's known-answer vectors for philox4x32_10."""
    for counter, key, want in R.KNOWN_ANSWERS:
        got = R.philox4x32_10(np.array(counter, np.uint64), np.array(key, np.uint64))
        assert got.dtype == np.uint32 and got.tolist() == list(want), ([hex(int(x)) for x in got], counter, key)
    # vectorised: the three at once
    got = R.philox4x32_10(np.array([c for c, _k, _o in R.KNOWN_ANSWERS], np.uint64), np.array([k for _c, k, _o in R.KNOWN_ANSWERS], np.uint64))
    assert got.tolist() == [list(o) for _c, _k, o in R.KNOWN_ANSWERS]


def test_the_header_on_the_host(tmp_path):
    """csrc/philox.hpp is host-compilable: g++ builds it (with the undefined-behaviour sanitizer linked in), it gives the known
    answers, the words of the restatement bit for bit, and the restatement's float32 normals within 8 ulp of the Box-Muller
    radius (libm's and numpy's logf / cosf / sinf need not round alike)."""
    cxx = shutil.which(os.environ.get("CXX", "g++"))
    assert cxx, "no C++ compiler"
    exe = str(tmp_path / "philox_main")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-fsanitize=undefined", "-static-libubsan", "-fno-sanitize-recover=all", "-Wall",
                        "-Werror", os.path.join(HERE, "philox_main.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "philox ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    lines = r.stdout.splitlines()
    kats = [[int(x, 16) for x in ln.split()[1:]] for ln in lines if ln.startswith("kat")]
    assert kats == [list(o) for _c, _k, o in R.KNOWN_ANSWERS]
    seed, call = 0x0123456789abcdef, (1 << 40) + 3
    rows = [ln.split()[1:] for ln in lines if ln.startswith("draw")]
    assert len(rows) == 300
    for purpose in range(3):
        mine = [r for r in rows if int(r[0]) == purpose]
        idx = np.array([int(r[1]) for r in mine])
        w = R.words(seed, call, purpose, idx)
        assert w.tolist() == [[int(x, 16) for x in r[2:6]] for r in mine]
        eps, rad = R.normals(seed, call, purpose, idx, np.float32)
        got = np.array([[float.fromhex(x) for x in r[6:9]] for r in mine])
        assert (np.abs(got - eps.astype(np.float64)) <= 8 * 2.0 ** -24 * rad.astype(np.float64)).all()
        # ... and the float32 normals are the float64 ones of the same bits within the argument's rounding: 2 pi u2 is off by
        # up to 2 pi (2^-24 + the 2.8e-8 of float32's 2 pi), times the radius
        e64, r64 = R.normals(seed, call, purpose, idx, np.float64)
        assert (np.abs(eps - e64) <= (2 * math.pi * (2.0 ** -24 + 2.8e-8) + 4 * 2.0 ** -24) * r64).all()


def test_stored_e32_matches_a_fresh_measurement():
    """tests/golden/mcmc/e32.json (python -m tests.mcmc_ref) is what a fresh measurement gives: the restatement is
    deterministic numpy, so within 10 %, the tolerance tests/test_gaussian_field_cpu.py uses for the field's file; and every
    4 x e32 is far below 1."""
    stored, fresh = R.load_e32(), R.measure_e32()

    def walk(a, b, path):
        assert type(a) is type(b), path
        if isinstance(a, dict):
            assert sorted(a) == sorted(b), path
            for k in a:
                walk(a[k], b[k], path + (k,))
        else:
            assert abs(a - b) <= 0.1 * b, (path, a, b)
            assert 0 <= 4 * a < 1e-4, (path, a)

    walk(stored, fresh, ())
    assert sorted(stored["noise"]) == sorted("p%d" % P for P in R.NOISE_P)
    assert sorted(stored["raw_density"]) == sorted(stored["round_trip"]) == sorted("p%d" % P for P in R.RELOC_P)


def test_sampler_counts_are_binomial():
    """20 000 draws on 50 weights spanning 10^6 : 1: every weight whose expected count is at least 50 is drawn within 5
    binomial standard deviations of it."""
    g = np.random.RandomState(9)
    w = np.exp(g.uniform(0.0, math.log(1e6), 50)).astype(np.float32)
    w[0], w[1] = 1.0, 1e6
    q = R.integer_weights(w)
    assert all(v >= 1 for v in q) and max(q) == 1 << 32
    cdf = list(np.cumsum(np.array(q, dtype=object)))
    T, n = cdf[-1], 20000
    src = R.draw(cdf, T, seed=5, call=11, first=0, count=n)
    counts = np.bincount(src, minlength=50)
    assert counts.sum() == n
    p = np.array([v / T for v in q], np.float64)
    checked = 0
    for i in range(50):
        if n * p[i] >= 50:
            checked += 1
            assert abs(counts[i] - n * p[i]) <= 5 * math.sqrt(n * p[i] * (1 - p[i])), (i, counts[i], n * p[i])
    assert checked >= 10
    # the integer weights are the float ratios: p is w / sum(w) to float32 accuracy
    assert np.allclose(p, w.astype(np.float64) / w.astype(np.float64).sum(), rtol=1e-6, atol=2.0 ** -32)


def test_normals_have_mean_0_and_variance_1():
    n = 40000
    eps, _rad = R.normals(0, 0, R.NOISE, np.arange((n + 2) // 3), np.float32)
    z = eps.reshape(-1)[:n].astype(np.float64)
    print("mean %.4f, variance %.4f" % (z.mean(), z.var()))
    assert abs(z.mean()) <= 5 / math.sqrt(n)
    assert abs(z.var() - 1) <= 5 * math.sqrt(2 / n)
    assert np.isfinite(z).all()


def test_plan_and_emit_of_the_restatement():
    """The bookkeeping of the restated sampler on the shared cases: slots, sources, counts and what each row is made of."""
    for P in (1, 2, 65):
        for kind in R.CASES:
            c = R.relocation_case(P, kind)
            rho = R.activate32(c["raw"])[0]
            for n_new in (0, 3):
                pl = R.plan(c["raw"], rho, c["weights"], c["dead_density"], n_new, seed=2, call=P)
                em = R.emit(pl, rho, n_new)
                slots = pl["D"] + n_new
                assert pl["dead"].sum() == pl["D"] and pl["draws"].sum() == (slots if pl["T"] else 0)
                assert (pl["sources"][slots:] == -1).all()
                if pl["T"]:
                    src = pl["sources"][:slots]
                    assert (src >= 0).all() and (pl["w"][src] > 0).all() and not pl["dead"][src].any()
                    assert em["fresh"].sum() == slots + (pl["draws"] >= 1).sum()
                    assert (em["copies"][em["fresh"]] == pl["draws"][em["src"][em["fresh"]]] + 1).all()
                else:
                    assert (pl["sources"] == -1).all() and em["fresh"].sum() == n_new
                    assert (em["density"][P:] == -100.0).all() and (em["src"][P:] == np.arange(n_new) % P).all()
            if kind == "nan_xyz":
                assert pl["dead"][P // 3]
            if kind == "wide":
                assert 1 in pl["q"] or P < 3
            if kind == "one_alive" and P > 1:
                pl = R.plan(c["raw"], rho, None, 0.005, 0)
                assert pl["draws"][P // 2] == P - 1 == pl["D"]


def test_parser_has_the_strategy_flags():
    from r2_gaussian_amd import train as TR
    a = TR.build_parser().parse_args(["-s", "x"])
    assert a.densify_strategy == "threshold" and a.dead_density == 0.005 and a.cap_max is None
    assert (a.lambda_density_l1, a.lambda_scale_l1) == (0.01, 0.01)
    a = TR.build_parser().parse_args(["-s", "x", "--densify_strategy", "mcmc", "--cap_max", "2000", "--dead_density", "0.01"])
    assert a.densify_strategy == "mcmc" and int(a.cap_max) == 2000 and a.dead_density == 0.01
    with pytest.raises(SystemExit):
        TR.build_parser().parse_args(["-s", "x", "--densify_strategy", "both"])
    opt = TR.OptimizationParams(densify_strategy="mcmc", cap_max=1700)
    assert opt.cap_max == 1700 and opt.dead_density == 0.005
