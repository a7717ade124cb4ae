"""GPU: r2_gaussian_noise and r2_relocate_plan / r2_relocate_emit (csrc/gaussian_mcmc.hip) through r2_gaussian_amd.mcmc against
the restatement of their contract (tests/mcmc_ref.py): the noise within 4 x the scene's measured float32 error of the float64
restatement fed the same Philox bits; the sampler's sources and counts EXACTLY the integer restatement's; every copied word bit
for bit; the split densities within 4 x their measured error; the exact operators (field.query_points,
gaussian_projector.project_gaussians) unchanged by a relocation without spread.

The activated arrays both sides start from are the device's own (gaussians.activate), so that the integer decisions -- dead or
alive, the integer weights -- are made on identical float32 words."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import mcmc_ref as R

pytestmark = pytest.mark.gpu
E32 = R.load_e32()
ULP = 2.0 ** -24
BIG_P = 2 * R.SCAN_TILE + 5   # more than two tiles of the 64-bit scan (R2_RELOCATE_SCAN_TILE = 4096): carries across workgroups
assert BIG_P in R.RELOC_P


def _dev(raw, gpu):
    return {n: torch.from_numpy(raw[n]).to(gpu) for n in R.NAMES}


def _activate(p):
    from r2_gaussian_amd.gaussians import activate
    return activate(p["density"], p["scaling"], p["rotation"], None)


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and bool(torch.equal(_bits(a), _bits(b)))


# ------------------------------------------------------------------------------------------------------ the noise
@pytest.mark.parametrize("P", R.NOISE_P)
def test_noise_against_float64(gpu, P):
    from r2_gaussian_amd import mcmc as MC
    p = _dev(R.cloud(P, 500 + P), gpu)
    d, s, q = _activate(p)
    lr = 2e-4 * R.NOISE_LR
    xyz = torch.zeros((P, 3), device=gpu)
    assert MC.position_noise(xyz, d, s, q, lr, seed=3, call=P) is xyz
    got = xyz.cpu().numpy().astype(np.float64)            # 0 + Delta: the kernel's Delta itself
    ref = R.noise(np.float64, d.cpu().numpy(), s.cpu().numpy(), q.cpu().numpy(), lr, seed=3, call=P)
    e32 = E32["noise"]["p%d" % P]
    tol = np.maximum(4 * e32 * ref["norm"], 8 * ULP * ref["floor"])
    err = np.abs(got - ref["delta"])
    print("P %d: worst error / norm %.3e (e32 %.3e), largest |Delta| %.3e" % (P, (err / ref["norm"]).max(), e32, np.abs(got).max()))
    assert (err <= tol).all()
    assert np.abs(got).max() > 0
    # in place on a cloud that is somewhere: one float32 addition of that Delta, bit for bit
    xyz2 = p["xyz"].clone()
    MC.position_noise(xyz2, d, s, q, lr, seed=3, call=P)
    assert _same_bits(xyz2, p["xyz"] + xyz)
    # the same (seed, call): the same bits; another seed or another call: other bits
    for seed, call, same in ((3, P, True), (4, P, False), (3, P + 1, False), (3, P + (1 << 32), False), (3 + (1 << 32), P, False)):
        again = torch.zeros((P, 3), device=gpu)
        MC.position_noise(again, d, s, q, lr, seed=seed, call=call)
        assert _same_bits(again, xyz) == same, (seed, call)


def test_noise_skips_unusable_rows_and_fades_with_density(gpu):
    from r2_gaussian_amd import mcmc as MC
    P = 65
    p = _dev(R.cloud(P, 500 + P), gpu)
    d, s, q = _activate(p)
    s, d, q = s.clone(), d.clone(), q.clone()
    s[7, 1], d[20, 0], q[64, 3] = float("nan"), float("inf"), float("nan")
    xyz = torch.zeros((P, 3), device=gpu)
    MC.position_noise(xyz, d, s, q, 100.0, call=1)
    moved = (xyz != 0).any(1).cpu().numpy()
    assert not moved[[7, 20, 64]].any() and moved.sum() == P - 3
    xyz = p["xyz"].clone()
    MC.position_noise(xyz, d, s, q, 100.0, call=1)
    assert bool(torch.equal(_bits(xyz)[[7, 20, 64]], _bits(p["xyz"])[[7, 20, 64]])) and not _same_bits(xyz, p["xyz"])
    # the same row, the same bits of randomness, two densities: 100 tau against 0
    one = {k: v[:1].contiguous() for k, v in zip(("d", "s", "q"), _activate(p))}
    out = []
    for rho in (0.0, 100 * R.TAU):
        x = torch.zeros((1, 3), device=gpu)
        MC.position_noise(x, torch.full((1, 1), rho, device=gpu), one["s"], one["q"], 100.0, density_threshold=R.TAU,
                          sharpness=R.KAPPA, call=5)
        out.append(x.cpu().numpy().astype(np.float64))
    assert np.abs(out[0]).max() > 0
    assert (np.abs(out[1]) < np.exp(-40.0) * np.abs(out[0])).all()
    # gate(0) is the method's sigmoid(100 * 0.005) = sigmoid(kappa)
    ref = R.noise(np.float64, np.zeros((1, 1), np.float32), one["s"].cpu().numpy(), one["q"].cpu().numpy(), 100.0, call=5)
    assert (np.abs(out[0] - ref["delta"]) <= 1e-4 * ref["norm"]).all()


# ------------------------------------------------------------------------------------------------------ relocation
def _relocate(gpu, c, n_new, P, spread=0.0, counts=True):
    from r2_gaussian_amd import mcmc as MC
    g = torch.Generator().manual_seed(P + n_new)
    p = _dev(c["raw"], gpu)
    moments = {n: (torch.randn(p[n].shape, generator=g).to(gpu), torch.rand(p[n].shape, generator=g).to(gpu)) for n in R.NAMES}
    stats = tuple((torch.rand(P, generator=g) + 0.5).to(gpu) for _ in range(3))
    act = _activate(p)
    w = None if c["weights"] is None else torch.from_numpy(c["weights"]).to(gpu)
    out = MC.relocate(p, moments, stats, c["dead_density"], n_new=n_new, weights=w, spread=spread, seed=1, call=P, counts=counts,
                      activated=act)
    return p, moments, stats, act, out


def _check_relocation(gpu, P, kind, n_new):
    c = R.relocation_case(P, kind)
    p, moments, stats, act, (np_, nm, ns, info) = _relocate(gpu, c, n_new, P)
    rho = act[0].cpu().numpy()
    pl = R.plan(c["raw"], rho, c["weights"], c["dead_density"], n_new, seed=1, call=P)
    em = R.emit(pl, rho, n_new, np.float64)
    tag = (P, kind, n_new)
    # the sampler: exactly the integer restatement
    assert np.array_equal(info["sources"].cpu().numpy(), pl["sources"]), tag
    assert np.array_equal(info["draws"].cpu().numpy(), pl["draws"]), tag
    assert (info["dead"], info["alive"], info["drawable"]) == (pl["D"], P - pl["D"], int((pl["w"] > 0).sum())), tag
    assert info["P"] == P + n_new == np_["xyz"].shape[0]
    src = torch.from_numpy(em["src"]).to(gpu)
    fresh = torch.from_numpy(em["fresh"]).to(gpu)
    # copied columns: bit for bit (a NaN included)
    for n in ("xyz", "scaling", "rotation"):
        assert _same_bits(np_[n], p[n][src]), tag + (n,)
    dens = np_["density"][:, 0]
    assert bool(torch.equal(_bits(dens)[~fresh], _bits(p["density"][:, 0][src])[~fresh])), tag
    want = em["density"][em["fresh"]]
    got = dens[fresh].cpu().numpy().astype(np.float64)
    if pl["T"] == 0:
        assert (got == -100.0).all() and em["fresh"].sum() == n_new, tag
    else:
        e32 = E32["raw_density"]["p%d" % P]
        assert np.isfinite(got).all() and (np.abs(got - want) <= 4 * e32 * (1 + np.abs(want))).all(), tag
    # moments and statistics: zero exactly on sources and slots, untouched elsewhere
    for n in R.NAMES:
        for k in range(2):
            new, old = nm[n][k], moments[n][k][src]
            assert bool((new[fresh] == 0).all()) and bool(torch.equal(_bits(new)[~fresh], _bits(old)[~fresh])), tag + (n, k)
    for k in range(3):
        new, old = ns[k], stats[k][src]
        assert bool((new[fresh] == 0).all()) and bool(torch.equal(_bits(new)[~fresh], _bits(old)[~fresh])), tag + ("stat", k)
    # a second call: the same bits
    _p, _m, _s, _a, (np2, nm2, ns2, info2) = _relocate(gpu, c, n_new, P, counts=False)
    assert torch.equal(info2["sources"], info["sources"]) and torch.equal(info2["draws"], info["draws"])
    for n in R.NAMES:
        assert _same_bits(np2[n], np_[n]) and _same_bits(nm2[n][0], nm[n][0]) and _same_bits(nm2[n][1], nm[n][1]), tag + (n,)
    assert all(_same_bits(a, b) for a, b in zip(ns2, ns))
    return pl, em


@pytest.mark.parametrize("P", R.RELOC_P)
def test_relocation_against_the_integer_restatement(gpu, P):
    """Every case of tests/mcmc_ref.relocation_case with 0, 1 and 70 appended rows, and nothing drawable with 3."""
    seen = set()
    for kind in R.CASES:
        for n_new in (0, 1, 70):
            pl, em = _check_relocation(gpu, P, kind, n_new)
            seen.add((pl["T"] > 0, pl["D"] > 0))
            if kind == "none_dead":
                assert pl["D"] == 0 and pl["draws"].sum() == n_new
            if kind == "all_dead":
                assert pl["T"] == 0 and pl["D"] == P
            if kind == "one_alive" and n_new == 0 and P > 1:
                assert pl["draws"][P // 2] == P - 1     # n = P - 1
            if kind == "wide" and P >= 63:
                assert 1 in pl["q"] and max(pl["q"]) == 1 << 32
            if kind == "nan_xyz":
                assert pl["dead"][P // 3]
    pl, em = _check_relocation(gpu, P, "all_dead", 3)
    assert pl["T"] == 0 and (em["src"][P:] == np.arange(3) % P).all()
    assert (True, False) in seen and (False, True) in seen and ((True, True) in seen or P == 1)


def test_relocation_without_state_and_without_activations(gpu):
    """moments = None, stats = None, and the activations computed by relocate itself: the same rows."""
    from r2_gaussian_amd import mcmc as MC
    P, n_new = 257, 9
    c = R.relocation_case(P, "mixed")
    p, _m, _s, _act, (want, _nm, _ns, info) = _relocate(gpu, c, n_new, P, counts=False)
    got, gm, gs, ginfo = MC.relocate(p, None, None, c["dead_density"], n_new=n_new, seed=1, call=P)
    assert gm is None and gs is None and torch.equal(ginfo["sources"], info["sources"])
    for n in R.NAMES:
        assert _same_bits(got[n], want[n]), n
    with pytest.raises(ValueError):
        MC.relocate(p, None, None, 0.005, n_new=-1)
    with pytest.raises(ValueError):
        MC.relocate(p, None, None, 0.005, spread=-1.0)


def test_relocation_preserves_the_field_and_the_projection(gpu):
    """spread = 0: n + 1 copies of density rho / (n + 1) are the Gaussian.  field.query_points at 200 points and
    project_gaussians on one 16 x 16 view before and after, within 4 x (the scene's field e32 + its round trip's e32) of the
    float64 sum of |terms|.  The rows that move carry an exact zero density (tests/mcmc_ref.field_scene)."""
    from r2_gaussian_amd import mcmc as MC
    from r2_gaussian_amd import projector
    from r2_gaussian_amd.field import query_points
    from r2_gaussian_amd.gaussian_projector import project_gaussians
    from tests import gaussian_field_ref as F
    from tests import gaussian_project_ref as PR
    raw, pts = R.field_scene()
    p = _dev(raw, gpu)
    act = _activate(p)
    new, _m, _s, info = MC.relocate(p, None, None, 0.005, n_new=R.FIELD_N_NEW, seed=0, call=7, counts=True, activated=act)
    assert info["dead"] > 50 and info["P"] == 300 + R.FIELD_N_NEW and int((info["draws"] >= 1).sum()) > 20
    act2 = _activate(new)
    dead = act[0][:, 0] <= 0.005
    assert bool((act[0][dead] == 0).all()) and bool((act2[0] > 0).all())
    tol = 4 * (E32["field"]["field"] + E32["field"]["round_trip"])
    cpu = [t.cpu().numpy() for t in (p["xyz"],) + tuple(act)]
    points = torch.from_numpy(pts).to(gpu)
    before = query_points(points, p["xyz"], *act).cpu().numpy().astype(np.float64)
    after = query_points(points, new["xyz"], *act2).cpu().numpy().astype(np.float64)
    ref = F.field64(pts, *cpu)
    print("field: worst |after - before| / sum|terms| %.3e, allowed %.3e" % (
        (np.abs(after - before)[ref["abs"] > 0] / ref["abs"][ref["abs"] > 0]).max(), tol))
    assert ref["abs"].max() > 0.1 and (np.abs(after - before) <= tol * ref["abs"] + F.FLOOR).all()
    views = PR._views("cone", 1, (16, 16))
    rays = projector.ray_params(views, (1.0, 1.0, 1.0), (0.0, 0.0, 0.0), (1, 1, 1))
    img0 = project_gaussians(views, p["xyz"], *act).cpu().numpy().astype(np.float64)
    img1 = project_gaussians(views, new["xyz"], *act2).cpu().numpy().astype(np.float64)
    r64 = PR.project64(rays, True, 16, 16, *cpu)
    print("projection: worst |after - before| / sum|terms| %.3e" % (np.abs(img1 - img0)[r64["abs"] > 0] / r64["abs"][r64["abs"] > 0]).max())
    assert r64["abs"].max() > 0.01 and (np.abs(img1 - img0) <= tol * r64["abs"] + PR.FLOOR).all()


def test_spread_moves_the_slots_and_only_them(gpu):
    P, n_new = 257, 30
    c = R.relocation_case(P, "mixed")
    p, _m, _s, act, (new, _nm, _ns, info) = _relocate(gpu, c, n_new, P, spread=1.0, counts=False)
    rho, s, q = (t.cpu().numpy() for t in act)
    pl = R.plan(c["raw"], rho, None, 0.005, n_new, seed=1, call=P)
    em = R.emit(pl, rho, n_new)
    assert np.array_equal(info["sources"].cpu().numpy(), pl["sources"])
    slot = em["slot"] >= 0
    src = torch.from_numpy(em["src"]).to(gpu)
    got, base = new["xyz"], p["xyz"][src]
    keep = torch.from_numpy(~slot).to(gpu)
    assert bool(torch.equal(_bits(got)[keep], _bits(base)[keep]))             # sources and untouched rows do not move
    assert bool((got[~keep] != base[~keep]).any(1).all()) and slot.sum() == pl["D"] + n_new > 50
    for n in ("scaling", "rotation"):
        assert _same_bits(new[n], p[n][src])
    # the displacement is spread * R S eps of the source, eps of (slot, purpose 2, call): against float64 from the same bits, within
    # 4 x the normals' measured error (the noise's e32) of sum_k |R_jk| s_k radius_k, plus the rounding of the sum itself
    want = R.spread_xyz(c["raw"]["xyz"], s, q, em, 1.0, seed=1, call=P, dtype=np.float64)
    k = np.nonzero(slot)[0]
    rad = R.normals(1, P, R.SPREAD, em["slot"][k], np.float64)[1]
    Rabs = np.abs(R.rot(q[em["src"][k]].astype(np.float64)))
    norm = np.einsum("pjk,pk->pj", Rabs, s[em["src"][k]].astype(np.float64) * rad)
    err = np.abs(got.cpu().numpy().astype(np.float64) - want)[k]
    assert (err <= 4 * max(E32["noise"].values()) * norm + 2 * ULP * np.abs(want[k])).all()


# ------------------------------------------------------------------------------------------------------ argument errors
def test_argument_errors(gpu):
    from r2_gaussian_amd import _lib
    from r2_gaussian_amd._boundary import call, ptr_table, workspace
    P, n_new = 10, 2
    p = _dev(R.cloud(P, 1), gpu)
    d, s, q = _activate(p)
    ps = [p[n] for n in R.NAMES]
    out = [torch.empty((P + n_new, w), device=gpu) for w in R.WIDTHS]
    sources = torch.empty(P + n_new, dtype=torch.int32, device=gpu)
    draws = torch.empty(P, dtype=torch.int32, device=gpu)
    nbytes = int(_lib.lib().r2_relocate_workspace_bytes(P, n_new))
    assert nbytes > 0 and _lib.lib().r2_relocate_workspace_bytes(0, 0) == 0
    ws = workspace(nbytes, gpu)
    zero = C.c_ulonglong(0)

    def plan(P=P, n_new=n_new, params=ptr_table(ps), dens=d, sources=sources, draws=draws, ws=ws, nbytes=nbytes):
        return call("r2_relocate_plan", gpu, P, n_new, params, dens, None, 0.005, zero, zero, sources, draws, ws, nbytes, None)

    def emit(P=P, n_new=n_new, params=ptr_table(ps), dens=d, sources=sources, draws=draws, ws=ws, nbytes=nbytes,
             outs=ptr_table(out), spread=0.0, scal=s):
        return call("r2_relocate_emit", gpu, P, n_new, params, None, None, dens, scal, q, None, None, None, spread, zero, zero,
                    sources, draws, ws, nbytes, outs, None, None, None, None, None)

    assert plan() == 0 and emit() == 0                     # the calls themselves are sound
    assert plan(P=0, n_new=0) == 0 and emit(P=0, n_new=0) == 0
    bad = [lambda: plan(P=-1), lambda: plan(n_new=-1), lambda: plan(P=0, n_new=1), lambda: plan(params=None), lambda: plan(dens=None),
           lambda: plan(params=ptr_table([ps[0], None, ps[2], ps[3]])), lambda: plan(sources=None), lambda: plan(draws=None),
           lambda: plan(ws=None), lambda: plan(nbytes=nbytes - 1),
           lambda: emit(P=-1), lambda: emit(n_new=-1), lambda: emit(P=0, n_new=1), lambda: emit(params=None), lambda: emit(dens=None),
           lambda: emit(outs=None), lambda: emit(outs=ptr_table([out[0], out[1], None, out[3]])), lambda: emit(sources=None),
           lambda: emit(draws=None), lambda: emit(ws=None), lambda: emit(nbytes=nbytes - 1), lambda: emit(spread=-1.0),
           lambda: emit(spread=0.5, scal=None)]
    for i, f in enumerate(bad):
        with pytest.raises(_lib.R2HipError):
            f()
            pytest.fail("call %d was accepted" % i)
    xyz = torch.zeros((P, 3), device=gpu)
    noise = lambda P=P, xyz=xyz, d=d, lr=1.0, tau=0.005, kappa=0.5: call("r2_gaussian_noise", gpu, P, xyz, d, s, q, lr, tau, kappa, zero, zero)
    assert noise() == 0 and noise(P=0) == 0
    for f in (lambda: noise(P=-1), lambda: noise(xyz=None), lambda: noise(d=None), lambda: noise(lr=-1.0), lambda: noise(lr=float("nan")),
              lambda: noise(tau=0.0), lambda: noise(kappa=-1.0)):
        with pytest.raises(_lib.R2HipError):
            f()
    torch.cuda.synchronize()
