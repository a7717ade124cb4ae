"""Restatement of the relocation / position-noise contract (include/r2hip.h: r2_gaussian_noise, r2_relocate_plan,
r2_relocate_emit; csrc/philox.hpp, csrc/gaussian_mcmc.hip), the scenes its tests share, and the measured float32 error the GPU
tolerances are taken from.  Host only; the product never imports this file.

* ``philox4x32_10`` / ``words``: Philox4x32-10 in numpy (uint64 products), the published known answers in ``KNOWN_ANSWERS``;
* ``normals``: the Box-Muller normals of an index, in float32 as the kernels form them or in float64 from the same bits;
* ``noise``: Delta of r2_gaussian_noise in float64, or in float32 in the kernel's operation order, with the normaliser
  N_j = lr gate sum_k |R_jk| s_k^2 sum_l |R_lk| r_l (r_l = the Box-Muller radius behind eps_l: the float32 error of
  r cos(2 pi u) scales with r, not with the value);
* ``plan``: the sampler in Python integers (classification, integer weights, prefix sum, draws, counts): exact;
* ``emit``: what every output row is made of, and the raw density of the split rows in float64 or in the kernel's order.

``python -m tests.mcmc_ref`` writes tests/golden/mcmc/e32.json: per scene the largest error of the float32 restatement against
float64 -- "noise": |Delta32 - Delta64| / N; "raw_density": |d32 - d64| / (1 + |d64|) of the raw densities after relocation;
"round_trip": |(n + 1) softplus32(d32) - rho| / rho, what a split does to the activated density; "field": on the scene of
the field test, the field's own float32 error (tests/gaussian_field_ref.py's measure), the same after relocation against the
float64 field of the cloud before it, and that relocation's round trip.  The GPU tests allow 4 x these, the project's
convention.
"""
import bisect
import json
import math
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mcmc", "e32.json")
M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
NOISE, DRAW, SPREAD = 0, 1, 2
SCAN_TILE = 4096            # R2_RELOCATE_SCAN_TILE: elements per workgroup of the 64-bit scan
NOISE_P = (1, 63, 64, 65, 1000)
RELOC_P = (1, 2, 63, 64, 65, 257, 1000, 2 * SCAN_TILE + 5)
TAU, KAPPA, NOISE_LR = 0.005, 0.5, 5e5
FIELD_N_NEW = 15
WIDTHS = (3, 1, 3, 4)
NAMES = ("xyz", "density", "scaling", "rotation")

KNOWN_ANSWERS = (   # Random123's kat_vectors: counter, key, output
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
)


# ------------------------------------------------------------------------------------------------------ the generator
def philox4x32_10(counter, key):
    """counter [..., 4], key [..., 2] (broadcast against each other) -> [..., 4] uint32."""
    c = [np.asarray(counter, np.uint64)[..., j] for j in range(4)]
    k = [np.asarray(key, np.uint64)[..., j] for j in range(2)]
    mask = np.uint64(0xFFFFFFFF)
    s32 = np.uint64(32)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        c = [(p1 >> s32) ^ c[1] ^ k[0], p1 & mask, (p0 >> s32) ^ c[3] ^ k[1], p0 & mask]
        k = [(k[0] + np.uint64(W0)) & mask, (k[1] + np.uint64(W1)) & mask]
    return np.stack(np.broadcast_arrays(*c), -1).astype(np.uint32)


def words(seed, call, purpose, index):
    """The four words of (index, purpose, call) under the key `seed`: index [N] -> [N, 4] uint32."""
    index = np.asarray(index, np.uint64).reshape(-1)
    ctr = np.empty((index.shape[0], 4), np.uint64)
    ctr[:, 0], ctr[:, 1], ctr[:, 2], ctr[:, 3] = index, purpose, call & 0xFFFFFFFF, (call >> 32) & 0xFFFFFFFF
    return philox4x32_10(ctr, np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], np.uint64))


def box_muller(a, b, dtype):
    """-> z0, z1, radius.  float32: every operation rounded on its own, in philox.hpp's order; float64: from the same bits."""
    u1 = ((a >> np.uint32(8)).astype(np.float64) + 1.0) * 2.0 ** -24
    u2 = (b >> np.uint32(8)).astype(np.float64) * 2.0 ** -24
    if dtype == np.float32:
        u1, u2 = u1.astype(np.float32), u2.astype(np.float32)   # exact
        r = np.sqrt(np.float32(-2.0) * np.log(u1))
        t = np.float32(6.283185307179586) * u2
        assert r.dtype == np.float32 and t.dtype == np.float32
        return r * np.cos(t), r * np.sin(t), r
    r = np.sqrt(-2.0 * np.log(u1))
    t = 2.0 * math.pi * u2
    return r * np.cos(t), r * np.sin(t), r


def normals(seed, call, purpose, index, dtype=np.float32):
    """-> eps [N, 3], radius [N, 3] (the Box-Muller radius behind each normal)."""
    w = words(seed, call, purpose, index)
    z0, z1, r01 = box_muller(w[:, 0], w[:, 1], dtype)
    z2, _, r2 = box_muller(w[:, 2], w[:, 3], dtype)
    return np.stack([z0, z1, z2], 1), np.stack([r01, r01, r2], 1)


def rot(q):
    """quat_to_rot of the quaternion as it comes, [P, 4] -> R [P, 3, 3] (row j, column i), in q's dtype."""
    r, x, y, z = (q[:, j] for j in range(4))
    one, two = q.dtype.type(1), q.dtype.type(2)
    return np.stack([np.stack([one - two * (y * y + z * z), two * (x * y - r * z), two * (x * z + r * y)], 1),
                     np.stack([two * (x * y + r * z), one - two * (x * x + z * z), two * (y * z - r * x)], 1),
                     np.stack([two * (x * z - r * y), two * (y * z + r * x), one - two * (x * x + y * y)], 1)], 1)


# ------------------------------------------------------------------------------------------------------ the noise
def noise(dtype, density, scaling, rotation, lr, tau=TAU, kappa=KAPPA, seed=0, call=0):
    """-> dict(delta [P,3] dtype, norm [P,3] float64, floor [P,3] float64 = lr gate sum_kl |R_jk| s_k^2 |R_lk|, touched [P]).
    Inputs are the float32 ACTIVATED arrays; tau, kappa are taken as the float32 values the entry receives."""
    rho = np.asarray(density, np.float32).reshape(-1)
    s = np.asarray(scaling, np.float32).reshape(-1, 3)
    q = np.asarray(rotation, np.float32).reshape(-1, 4)
    P = rho.shape[0]
    touched = np.isfinite(rho) & np.isfinite(s).all(1) & np.isfinite(q).all(1)
    tau, kappa = np.float32(tau), np.float32(kappa)
    with np.errstate(all="ignore"):
        eps, rad = normals(seed, call, NOISE, np.arange(P), dtype)
        if dtype == np.float32:
            gate = np.float32(1) / (np.float32(1) + np.exp(kappa * (rho / tau - np.float32(1))))
            lg = (float(lr) * gate.astype(np.float64)).astype(np.float32)
            R = rot(q)
            a = (R[:, 0, :] * eps[:, 0:1] + R[:, 1, :] * eps[:, 1:2]) + R[:, 2, :] * eps[:, 2:3]
            b = (s * s) * a
            d = (R[:, :, 0] * b[:, 0:1] + R[:, :, 1] * b[:, 1:2]) + R[:, :, 2] * b[:, 2:3]
            delta = lg[:, None] * d
            assert delta.dtype == np.float32
        else:
            rho64, s64 = rho.astype(np.float64), s.astype(np.float64)
            gate = 1.0 / (1.0 + np.exp(float(kappa) * (rho64 / float(tau) - 1.0)))
            R = rot(q.astype(np.float64))
            a = np.einsum("pki,pk->pi", R, eps)
            delta = (float(lr) * gate)[:, None] * np.einsum("pjk,pk->pj", R, s64 * s64 * a)
        R64 = np.abs(rot(q.astype(np.float64)))
        s64 = s.astype(np.float64)
        g64 = float(lr) / (1.0 + np.exp(float(kappa) * (rho.astype(np.float64) / float(tau) - 1.0)))
        rad64 = normals(seed, call, NOISE, np.arange(P), np.float64)[1]
        norm = g64[:, None] * np.einsum("pjk,pk->pj", R64, s64 * s64 * np.einsum("pki,pk->pi", R64, rad64))
        floor = g64[:, None] * np.einsum("pjk,pk->pj", R64, s64 * s64 * R64.sum(1))
    delta = np.where(touched[:, None], delta, 0).astype(dtype)
    return {"delta": delta, "norm": np.where(touched[:, None], norm, 0.0), "floor": np.where(touched[:, None], floor, 0.0),
            "touched": touched}


# ------------------------------------------------------------------------------------------------------ the sampler
def integer_weights(w):
    """w [P] float32, 0 for rows that are not drawable -> list of Python integers q."""
    w = np.asarray(w, np.float32)
    if not (w > 0).any():
        return [0] * w.shape[0]
    ratio = w / w.max()
    assert ratio.dtype == np.float32
    return [max(1, int(float(x) * 4294967296.0)) if x > 0 else 0 for x in ratio]


def draw(cdf, T, seed, call, first, count):
    """Sources of the slots first .. first + count - 1 by the contract's rule, Python integers throughout."""
    w = words(seed, call, DRAW, np.arange(first, first + count))
    out = []
    for a, b in zip(w[:, 0].tolist(), w[:, 1].tolist()):
        t = (((a << 32) | b) * T) >> 64
        out.append(bisect.bisect_right(cdf, t))   # the first i with cdf[i] > t
    return out


def plan(raw, density_act, weights, dead_density, n_new, seed=0, call=0):
    """-> dict(dead [P] bool, w [P] float32, q, cdf (lists of int), T, D, sources [P + n_new] int32, draws [P] int32)."""
    rho = np.asarray(density_act, np.float32).reshape(-1)
    P = rho.shape[0]
    fin = np.ones(P, bool)
    for n, width in zip(NAMES, WIDTHS):
        fin &= np.isfinite(np.asarray(raw[n], np.float32).reshape(P, width)).all(1)
    with np.errstate(invalid="ignore"):
        alive = fin & (rho > np.float32(dead_density)) & (rho < np.inf)
        wi = rho if weights is None else np.asarray(weights, np.float32).reshape(-1)
        w = np.where(alive & (wi > 0) & (wi < np.inf), wi, np.float32(0)).astype(np.float32)
    q = integer_weights(w)
    cdf, run = [], 0
    for v in q:
        run += v
        cdf.append(run)
    T, D = run, int((~alive).sum())
    sources = np.full(P + n_new, -1, np.int32)
    draws = np.zeros(P, np.int32)
    if T > 0 and D + n_new > 0:
        src = draw(cdf, T, seed, call, 0, D + n_new)
        sources[:D + n_new] = src
        draws = np.bincount(src, minlength=P).astype(np.int32)
    return {"dead": ~alive, "w": w, "q": q, "cdf": cdf, "T": T, "D": D, "sources": sources, "draws": draws}


def inv_softplus(x, dtype):
    """float32: the kernel's order (the quotient is the caller's float32; log(expm1()) in double, rounded once)."""
    x = np.asarray(x)
    with np.errstate(all="ignore"):
        d = np.where(x > 20, x.astype(np.float64), np.log(np.expm1(x.astype(np.float64))))
    return d.astype(dtype)


def softplus32(x):
    """r2_gaussian_activate's density activation in float32."""
    x = np.asarray(x, np.float32)
    with np.errstate(all="ignore"):
        return np.where(x > 20, x, np.log1p(np.exp(x))).astype(np.float32)


def emit(pl, density_act, n_new, dtype=np.float64):
    """What the rows of the output are made of.  -> dict(src [Pn] int64: the row whose xyz, scaling and rotation (and, for a
    row that is not fresh, everything else) it copies; fresh [Pn] bool: zero moments and statistics and a new raw density;
    slot [Pn] int64 (-1: none); density [Pn] dtype: the raw density of the fresh rows (nan elsewhere); copies [Pn]: n + 1)."""
    rho = np.asarray(density_act, np.float32).reshape(-1)
    P = rho.shape[0]
    Pn = P + n_new
    src = np.arange(Pn, dtype=np.int64)
    fresh = np.zeros(Pn, bool)
    slot = np.full(Pn, -1, np.int64)
    dens = np.full(Pn, np.nan, dtype)
    copies = np.ones(Pn, np.int64)
    if pl["T"] > 0:
        slot[:P][pl["dead"]] = np.arange(pl["D"])
        slot[P:] = pl["D"] + np.arange(n_new)
        has = slot >= 0
        src[has] = pl["sources"][slot[has]]
        fresh[has] = True
        fresh[:P] |= (~pl["dead"]) & (pl["draws"] >= 1)
        copies[fresh] = pl["draws"][src[fresh]].astype(np.int64) + 1
        if dtype == np.float32:
            x = rho[src[fresh]] / copies[fresh].astype(np.float32)
            assert x.dtype == np.float32
        else:
            x = rho[src[fresh]].astype(np.float64) / copies[fresh]
        dens[fresh] = inv_softplus(x, dtype)
    else:
        src[P:] = np.arange(n_new) % P
        fresh[P:] = True
        dens[P:] = -100.0
    return {"src": src, "fresh": fresh, "slot": slot, "density": dens, "copies": copies}


def spread_xyz(xyz, scaling_act, rotation_act, em, spread, seed=0, call=0, dtype=np.float32):
    """The xyz of every output row with spread: slots are displaced by spread * R S eps of their source, in the kernel's order."""
    xyz = np.asarray(xyz, np.float32)
    out = xyz[em["src"]].astype(dtype)
    k = np.nonzero(em["slot"] >= 0)[0]
    if spread > 0 and k.size:
        s = np.asarray(scaling_act, np.float32)[em["src"][k]].astype(dtype)
        R = rot(np.asarray(rotation_act, np.float32)[em["src"][k]].astype(dtype))
        eps = normals(seed, call, SPREAD, em["slot"][k], dtype)[0]
        v = s * eps
        d = (R[:, :, 0] * v[:, 0:1] + R[:, :, 1] * v[:, 1:2]) + R[:, :, 2] * v[:, 2:3]
        out[k] = out[k] + dtype(spread) * d
    return out


# ------------------------------------------------------------------------------------------------------ the shared scenes
def cloud(P, seed, dead_fraction=0.3):
    """RAW parameters of P Gaussians (exp scale activation, no bound): means in a cube of half-side 0.5, scales log-uniform in
    [0.01, 0.3], quaternions of norm 0.5 .. 2, activated densities log-uniform in [1e-4, 0.1] -- `dead_fraction` of them below
    the 0.005 of the tests.  -> dict name -> float32 array."""
    g = np.random.RandomState(seed)
    xyz = (g.rand(P, 3) * 2 - 1) * 0.5
    sc = np.log(np.exp(np.log(0.01) + g.rand(P, 3) * (np.log(0.3) - np.log(0.01))))
    q = g.randn(P, 4)
    q *= np.exp(g.uniform(np.log(0.5), np.log(2.0), (P, 1))) / np.linalg.norm(q, axis=1, keepdims=True)
    low = g.rand(P) < dead_fraction
    rho = np.where(low, np.exp(g.uniform(np.log(1e-4), np.log(4e-3), P)), np.exp(g.uniform(np.log(6e-3), np.log(0.1), P)))
    dens = np.log(np.expm1(rho))[:, None]
    return {n: np.ascontiguousarray(a, np.float32) for n, a in zip(NAMES, (xyz, dens, sc, q))}


def activate32(raw):
    """r2_gaussian_activate without a scale bound, in numpy float32: -> (density [P,1], scaling [P,3], rotation [P,4])."""
    q = raw["rotation"].astype(np.float64)
    n = np.maximum(np.sqrt((q * q).sum(1, keepdims=True)).astype(np.float32), np.float32(1e-12))
    with np.errstate(all="ignore"):
        return softplus32(raw["density"]), np.exp(raw["scaling"]).astype(np.float32), (raw["rotation"] / n).astype(np.float32)


CASES = ("mixed", "none_dead", "all_dead", "one_alive", "wide", "nan_xyz", "caller_weights")


def relocation_case(P, kind):
    """-> dict(raw, weights (None or [P] float32), dead_density): the cases of the relocation tests on P rows.
    mixed: about 30 % dead; none_dead; all_dead (nothing drawable: T = 0); one_alive: row P // 2 alone (n = P - 1 with no
    appended rows); wide: caller weights spanning 2^40 : 1, so that q = 1 occurs; nan_xyz: a NaN in one raw xyz of an
    otherwise alive row; caller_weights: zeros and an inf among the caller's weights."""
    raw = cloud(P, 1000 + P, dead_fraction={"none_dead": 0.0, "all_dead": 1.0, "one_alive": 1.0}.get(kind, 0.3))
    weights = None
    g = np.random.RandomState(77 + P)
    if kind == "one_alive":
        raw["density"][P // 2, 0] = np.float32(np.log(np.expm1(0.05)))
    elif kind == "wide":
        weights = np.exp2(-40.0 * g.rand(P)).astype(np.float32)
        weights[0], weights[-1] = 1.0, 2.0 ** -40
        raw["density"][[0, -1], 0] = np.float32(np.log(np.expm1(0.05)))   # both ends of the span are alive
    elif kind == "nan_xyz":
        raw["density"][P // 3, 0] = np.float32(np.log(np.expm1(0.05)))
        raw["xyz"][P // 3, 1] = np.nan
    elif kind == "caller_weights":
        weights = g.rand(P).astype(np.float32)
        weights[::3] = 0.0
        weights[P // 2] = np.inf
        weights[-1] = 0.7
    return {"raw": raw, "weights": weights, "dead_density": 0.005}


def field_scene():
    """The cloud and the 200 points of the field-preservation test: 300 Gaussians, about 30 % of them dead with a raw density
    of -200, whose activation is an exact float32 zero -- a dead row that still carries density takes it along when it moves,
    which is the method's intent and no rounding error, so the rows that move here carry none."""
    raw = cloud(300, 4242)
    raw["density"][softplus32(raw["density"]) < 0.005] = -200.0
    pts = ((np.random.RandomState(4243).rand(200, 3) * 2 - 1) * 0.6).astype(np.float32)
    return raw, pts


# ------------------------------------------------------------------------------------------------------ the measured error
def _worst(err, den):
    m = den > 0
    return float((np.abs(err)[m] / den[m]).max()) if m.any() else 0.0


def measure_noise(P):
    act = activate32(cloud(P, 500 + P))
    lr = 2e-4 * NOISE_LR
    a, b = noise(np.float32, *act, lr, seed=3, call=P), noise(np.float64, *act, lr, seed=3, call=P)
    return _worst(a["delta"].astype(np.float64) - b["delta"], b["norm"])


def measure_relocation(P):
    """-> (raw_density, round_trip) over the cases of P rows with 70 appended rows."""
    worst_d, worst_rt = 0.0, 0.0
    for kind in CASES:
        c = relocation_case(P, kind)
        rho = activate32(c["raw"])[0]
        pl = plan(c["raw"], rho, c["weights"], c["dead_density"], 70, seed=1, call=P)
        e32, e64 = emit(pl, rho, 70, np.float32), emit(pl, rho, 70, np.float64)
        f = e64["fresh"] & (pl["T"] > 0)
        if not f.any():
            continue
        d32, d64 = e32["density"][f].astype(np.float64), e64["density"][f]
        worst_d = max(worst_d, _worst(d32 - d64, 1.0 + np.abs(d64)))
        r = rho.reshape(-1)[e64["src"][f]].astype(np.float64)
        back = softplus32(e32["density"][f]).astype(np.float64) * e64["copies"][f]
        worst_rt = max(worst_rt, _worst(back - r, r))
    return worst_d, worst_rt


def measure_field():
    """-> dict(field, after, round_trip): tests/gaussian_field_ref.py's measure on the field scene before and after the
    relocation of the field test (FIELD_N_NEW appended rows, seed 0, call 7), and the density round trip of that relocation."""
    from tests import gaussian_field_ref as F
    raw, pts = field_scene()
    rho, s, q = activate32(raw)
    ref = F.field64(pts, raw["xyz"], rho, s, q)
    before = F.field32(pts, raw["xyz"], rho, s, q)
    pl = plan(raw, rho, None, 0.005, FIELD_N_NEW, seed=0, call=7)
    em = emit(pl, rho, FIELD_N_NEW, np.float32)
    act = softplus32(em["density"])
    dens = np.where(em["fresh"], act, rho.reshape(-1)[em["src"]]).astype(np.float32)
    after = F.field32(pts, raw["xyz"][em["src"]], dens[:, None], s[em["src"]], q[em["src"]])
    f = em["fresh"]
    r = rho.reshape(-1)[em["src"][f]].astype(np.float64)
    return {"field": _worst(before["val"].astype(np.float64) - ref["val"], ref["abs"]),
            "after": _worst(after["val"].astype(np.float64) - ref["val"], ref["abs"]),
            "round_trip": _worst(act[f].astype(np.float64) * em["copies"][f] - r, r)}


def measure_e32():
    out = {"noise": {"p%d" % P: measure_noise(P) for P in NOISE_P}, "raw_density": {}, "round_trip": {}}
    for P in RELOC_P:
        out["raw_density"]["p%d" % P], out["round_trip"]["p%d" % P] = measure_relocation(P)
    out["field"] = measure_field()
    return out


def load_e32():
    with open(GOLDEN) as f:
        return json.load(f)


if __name__ == "__main__":
    os.makedirs(os.path.dirname(GOLDEN), exist_ok=True)
    res = measure_e32()
    with open(GOLDEN, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print(json.dumps(res, indent=1, sort_keys=True))
