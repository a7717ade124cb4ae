"""densify_and_prune (r2_gaussian/gaussian/gaussian_model.py:430-556) as csrc/densify_ops.hip's header comment lays it out, stated
three times over plain numpy arrays:

``statement``   in float64, from the float32 inputs: the decisions of every row with the margin of every comparison, the layout of
                the result ([originals | clones | first children | second children], each in row order), the values, and for
                every computed value a first-order bound on what float32 arithmetic in the kernel's operation order (decide() in
                densify_ops.hip, the activations of cloud_model.hpp) may differ from it.
``restate32``   in numpy float32, operation for operation as the kernel has them and without fused operations: CPU only, to show
                that the bound is honest (it holds for an independent float32 evaluation) and, with ``mutate``, that the
                comparator notices the errors it is for.
``check``       the one comparator of the CPU and the GPU test.

The error model.  A value is carried as (v, e): v the float64 value, e a bound on |float32 result - v|.  Inputs are exact.  Every
``+ - * /`` and ``sqrtf`` adds half an ulp of its result, every ``expf``, ``logf``, ``log1pf`` and sigmoid two ulp of its result
(what tests/test_gaussian_step_gpu.py grants the activations against float64), and e goes through every operation to first order:
    a * b: |a| e_b + |b| e_a        a / b: e_a / |b| + |a| e_b / b^2        exp(a): exp(a) e_a        log(a): e_a / |a|
so the conditioning of each formula appears where it arises and nowhere as a constant:
    halved density   log(E - 1), E = exp(h):   e_E / (E - 1), with e_E = 2 ulp(E) and E / (E - 1) ~ 1 / h for a small h
    bounded child    log(t / (1 - t)), t = (y - lo) / range:   e_t / (t (1 - t)), with e_t ~ ulp(y) / (y - lo) of relative error
    child xyz        R v + p, three-term sums of products that may cancel:   the error is that of the terms, not of the sum
A product or sum that leaves float32's range becomes the infinity float32 makes of it; one that falls under the smallest normal
number carries that number as absolute error (it may be flushed).

A comparison ``quantity ? threshold`` has the margin |quantity - threshold| / max(|threshold|, tiny) in float64, and ``qerr``, the
bound of the float32 quantity in the same unit.  Where the float32 evaluation puts the quantity on the threshold EXACTLY (and
float64 agrees to within float32 rounding) the margin is 0 and the comparison is decided as equality -- the reference computes
in float32, so that is what it sees there.  Rows planted on a threshold are exact in float32 by construction (``edge_case``
asserts it); every other row of ``edge_case`` keeps every margin above 1e-4, a hundred times float32's rounding, and above four
times qerr, so its decisions are the same in any honest float32 evaluation.
"""
import numpy as np

NAMES = ("xyz", "density", "scaling", "rotation")
WIDTHS = {"xyz": 3, "density": 1, "scaling": 3, "rotation": 4}
ORIGINAL, CLONE, CHILD0, CHILD1 = 0, 1, 2, 3
F32 = np.float32
FLT_MAX, FLT_MIN = float(np.finfo(F32).max), float(np.finfo(F32).tiny)
TINY = 1e-30                       # the margin's floor for a zero threshold
DIV = F32(1.6)                     # 0.8 * N with N = 2 children, as the float32 the reference divides by
MARGIN = 1e-4                      # what every comparison of a row that is not planted keeps


# ------------------------------------------------------------------------------------------------ values with an error bound
def ulp(v):
    """Spacing of float32 at |v| (float64); at a non-finite v that of the largest finite number."""
    a = np.abs(np.asarray(v, np.float64))
    a = np.where(np.isfinite(a), np.minimum(a, FLT_MAX), FLT_MAX)
    return np.spacing(a.astype(F32)).astype(np.float64)


class E:
    """Float64 value v and a first-order bound e on the distance of the float32 result from it."""
    __slots__ = ("v", "e")

    def __init__(self, v, e=0.0):
        self.v = np.asarray(v, np.float64)
        self.e = np.broadcast_to(np.asarray(e, np.float64), self.v.shape).copy()

    @staticmethod
    def of(x):
        return x if isinstance(x, E) else E(x)

    @staticmethod
    def rounded(v, e, ulps=0.5):
        """The result of one float32 operation with exact value v and inherited error e."""
        with np.errstate(all="ignore"):
            over = np.abs(v) > FLT_MAX
            v = np.where(over, np.sign(v) * np.inf, v)
            e = np.where(over, 0.0, e + ulps * ulp(v))
            e = np.where((np.abs(v) < FLT_MIN) & (v != 0), e + FLT_MIN, e)
        return E(v, e)

    def __add__(self, o):
        o = E.of(o)
        with np.errstate(all="ignore"):
            return E.rounded(self.v + o.v, self.e + o.e)

    def __sub__(self, o):
        o = E.of(o)
        with np.errstate(all="ignore"):
            return E.rounded(self.v - o.v, self.e + o.e)

    def __rsub__(self, o):
        return E.of(o) - self

    def __mul__(self, o):
        o = E.of(o)
        with np.errstate(all="ignore"):
            return E.rounded(self.v * o.v, np.abs(self.v) * o.e + np.abs(o.v) * self.e)

    def __truediv__(self, o):
        o = E.of(o)
        with np.errstate(all="ignore"):
            return E.rounded(self.v / o.v, self.e / np.abs(o.v) + np.abs(self.v) * o.e / (o.v * o.v))

    def __rtruediv__(self, o):
        return E.of(o) / self

    def pow2(self, c):
        """Times a power of two: exact in float32."""
        return E(self.v * c, self.e * abs(c))

    def where(self, cond, other):
        other = E.of(other)
        return E(np.where(cond, self.v, other.v), np.where(cond, self.e, other.e))


def e_exp(a):
    with np.errstate(all="ignore"):
        v = np.exp(a.v)
        return E.rounded(v, v * a.e, 2.0)


def e_log(a):
    with np.errstate(all="ignore"):
        return E.rounded(np.log(a.v), a.e / np.abs(a.v), 2.0)


def e_log1p(a):
    with np.errstate(all="ignore"):
        return E.rounded(np.log1p(a.v), a.e / (1.0 + a.v), 2.0)


def e_sqrt(a):
    """sqrt over the interval [v - e, v + e], not to first order: the argument may have underflowed to nothing."""
    with np.errstate(all="ignore"):
        v = np.sqrt(a.v)
        lo, hi = np.sqrt(np.maximum(a.v - a.e, 0.0)), np.sqrt(a.v + a.e)
        e = np.where(np.isfinite(v), np.maximum(v - lo, hi - v), 0.0)
        return E.rounded(v, e)


def e_sigmoid(a):
    with np.errstate(all="ignore"):
        v = 1.0 / (1.0 + np.exp(-a.v))
        return E.rounded(v, v * (1.0 - v) * a.e, 2.0)


def e_softplus(a):
    """cloud_model.hpp softplus_f: x above 20 as it is."""
    return a.where(a.v > 20.0, e_log1p(e_exp(a)))


def e_max3(a):
    """fmaxf over the last axis of an E: exact, the bound is that of the elements."""
    return E(a.v.max(axis=-1), a.e.max(axis=-1))


# ------------------------------------------------------------------------------------------------ the inputs
def make_inputs(params, moments, max_radii2D, grad_accum, denom, normals, grad_thr, scale_thr, density_min, bbox, scale_bound=None,
                do_densify=True, max_screen_size=None, max_scale=None):
    """The arguments of densify.densify_and_prune as float32 numpy arrays / the float32 values the C ABI receives."""
    P = np.asarray(params["xyz"]).shape[0]
    inp = {n: np.ascontiguousarray(np.asarray(params[n], F32).reshape(P, WIDTHS[n])) for n in NAMES}
    inp["moments"] = None if moments is None else {
        n: tuple(np.ascontiguousarray(np.asarray(t, F32).reshape(P, WIDTHS[n])) for t in moments[n]) for n in NAMES}
    for k, t in (("max_radii2D", max_radii2D), ("grad_accum", grad_accum), ("denom", denom)):
        inp[k] = np.ascontiguousarray(np.asarray(t, F32).reshape(P))
    inp["normals"] = np.ascontiguousarray(np.asarray(normals, F32).reshape(2, P, 3))
    inp["grad_thr"], inp["scale_thr"], inp["density_min"] = F32(grad_thr), F32(scale_thr), F32(density_min)
    inp["bbox"] = np.asarray(bbox, F32).reshape(2, 3)
    inp["scale_bound"] = None if scale_bound is None else (F32(scale_bound[0]), F32(scale_bound[1]))
    inp["do_densify"] = bool(do_densify)
    inp["max_screen"], inp["max_scale"] = F32(max_screen_size or 0.0), F32(max_scale or 0.0)   # 0: off, the reference's None
    return inp


def _scale_cfg(inp):
    """bounded, range, lo as make_cfg (densify_ops.hip) forms them: the range is hi - lo subtracted in float32."""
    sb = inp["scale_bound"]
    if sb is None:
        return False, F32(0), F32(0)
    return True, F32(sb[1] - sb[0]), sb[0]


# ------------------------------------------------------------------------------------------------ float32, the kernel's order
def _quat_rot32(r, x, y, z, transpose=False):
    one, two = F32(1), F32(2)
    R = [[one - two * (y * y + z * z), two * (x * y - r * z), two * (x * z + r * y)],
         [two * (x * y + r * z), one - two * (x * x + z * z), two * (y * z - r * x)],
         [two * (x * z - r * y), two * (y * z + r * x), one - two * (x * x + y * y)]]
    return [[R[i][j] for i in range(3)] for j in range(3)] if transpose else R


MUTATIONS = ("grad_gt", "scale_lt", "density_le", "open_box", "screen_ge", "divide_by_1_5", "clone_full_density",
             "fresh_rows_take_moments", "stats_not_reset", "second_children_first", "transposed_rotation",
             "child_density_unhalved")


def decide32(inp, mutate=None):
    """decide() of densify_ops.hip for all rows at once in numpy float32.  ``mutate``: one of MUTATIONS, a kernel subtly wrong."""
    assert mutate is None or mutate in MUTATIONS, mutate
    with np.errstate(all="ignore"):
        bounded, rng, lo = _scale_cfg(inp)
        one = F32(1)
        softplus = lambda x: np.where(x > F32(20), x, np.log1p(np.exp(x)))            # noqa: E731
        inv_softplus = lambda y: np.log(np.exp(y) - one)                              # noqa: E731
        act = (lambda x: (one / (one + np.exp(-x))) * rng + lo) if bounded else np.exp

        def inv(y):
            if not bounded:
                return np.log(y)
            t = np.maximum((y - lo) / rng, F32(0))
            return np.log(t / (one - t))

        def outside(p):
            b = inp["bbox"]
            if mutate == "open_box":
                return ((p <= b[0]) | (p >= b[1])).any(axis=-1)
            return ((p < b[0]) | (p > b[1])).any(axis=-1)

        p, raw_d, mr = inp["xyz"], inp["density"][:, 0], inp["max_radii2D"]
        s = act(inp["scaling"])
        smax = np.maximum(np.maximum(s[:, 0], s[:, 1]), s[:, 2])
        dens = softplus(raw_d)
        g = inp["grad_accum"] / inp["denom"]
        g = np.where(g != g, F32(0), g)
        hot = (g > inp["grad_thr"] if mutate == "grad_gt" else g >= inp["grad_thr"]) & inp["do_densify"]
        small = smax < inp["scale_thr"] if mutate == "scale_lt" else smax <= inp["scale_thr"]
        clone, split = hot & small, hot & ~small
        half = inv_softplus(dens * F32(0.5))
        if mutate == "child_density_unhalved":     # an expm1-accurate clone, and the child's from the density as it was
            half = np.log(np.expm1(dens.astype(np.float64) * 0.5)).astype(F32)
        d_orig = np.where(clone & (mutate != "clone_full_density"), half, raw_d)
        q_dens = softplus(d_orig)
        big_screen = (inp["max_screen"] > 0) & (mr >= inp["max_screen"] if mutate == "screen_ge" else mr > inp["max_screen"])
        low_d = q_dens <= inp["density_min"] if mutate == "density_le" else q_dens < inp["density_min"]
        pruned = low_d | outside(p) | big_screen | ((inp["max_scale"] > 0) & (smax > inp["max_scale"]))
        q = inp["rotation"]
        n = np.sqrt(q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1] + q[:, 2] * q[:, 2] + q[:, 3] * q[:, 3])
        R = _quat_rot32(q[:, 0] / n, q[:, 1] / n, q[:, 2] / n, q[:, 3] / n, mutate == "transposed_rotation")
        d_child = inv_softplus(dens) if mutate == "child_density_unhalved" else inv_softplus(dens * F32(0.5))
        s_child = inv(s / (F32(1.5) if mutate == "divide_by_1_5" else DIV))
        a_child = act(s_child)
        q_child_dens = softplus(d_child)
        q_child_smax = np.maximum(np.maximum(a_child[:, 0], a_child[:, 1]), a_child[:, 2])
        low = (q_child_dens <= inp["density_min"] if mutate == "density_le" else q_child_dens < inp["density_min"]) | big_screen
        low = low | ((inp["max_scale"] > 0) & (q_child_smax > inp["max_scale"]))
        v = inp["normals"] * s[None]
        xyz_child = np.stack([R[j][0] * v[..., 0] + R[j][1] * v[..., 1] + R[j][2] * v[..., 2] + p[:, j] for j in range(3)], axis=-1)
        keep_child = split[None] & ~low[None] & ~np.stack([outside(xyz_child[0]), outside(xyz_child[1])])
    return dict(clone=clone, split=split, keep_orig=~split & ~pruned, keep_clone=clone & ~pruned, keep_child=keep_child,
                density_raw_orig=d_orig.astype(F32), child_xyz=xyz_child.astype(F32), child_density_raw=d_child.astype(F32),
                child_scaling_raw=s_child.astype(F32),
                q=dict(g=g, smax=smax, dens=q_dens, child_dens=q_child_dens, child_smax=q_child_smax, child_xyz=xyz_child))


def restate32(inp, mutate=None):
    """The result of densify_and_prune in numpy float32, in the kernel's operation order: the dict ``check`` takes."""
    d = decide32(inp, mutate)
    segs = [(ORIGINAL, d["keep_orig"]), (CLONE, d["keep_clone"]), (CHILD0, d["keep_child"][0]), (CHILD1, d["keep_child"][1])]
    counts = tuple(int(k.sum()) for _kind, k in segs)
    if mutate == "second_children_first":
        segs = [segs[0], segs[1], segs[3], segs[2]]
    src = np.concatenate([np.nonzero(k)[0] for _kind, k in segs])
    kind = np.concatenate([np.full(int(k.sum()), kd) for kd, k in segs])
    child = kind >= CHILD0
    ch = np.where(child, kind - CHILD0, 0)
    out = {"xyz": np.where(child[:, None], d["child_xyz"][ch, src], inp["xyz"][src]),
           "density": np.where(child, d["child_density_raw"][src], d["density_raw_orig"][src])[:, None],
           "scaling": np.where(child[:, None], d["child_scaling_raw"][src], inp["scaling"][src]),
           "rotation": inp["rotation"][src]}
    out["moments"] = None
    if inp["moments"] is not None:
        keep = (kind == ORIGINAL) | (mutate == "fresh_rows_take_moments")
        out["moments"] = {n: tuple(np.where(keep[:, None], t[src], F32(0)) for t in inp["moments"][n]) for n in NAMES}
    reset = inp["do_densify"] and mutate != "stats_not_reset"
    out["max_radii2D"] = inp["max_radii2D"][src]
    out["grad_accum"] = np.zeros(len(src), F32) if reset else inp["grad_accum"][src]
    out["denom"] = np.zeros(len(src), F32) if reset else inp["denom"][src]
    out["counts"] = counts
    return out


# ------------------------------------------------------------------------------------------------ float64, the statement
class _Comparisons:
    """Every ``quantity ? threshold`` of the statement: decided in float64, as equality where float32 lands on the threshold."""

    def __init__(self):
        self.margin, self.qerr = {}, {}

    def gt(self, name, q, q32, thr, entered=True):
        """q ? thr per element -> (gt, ge, lt), all false for a NaN; records the margin and the float32 quantity's bound, both over max(|thr|, tiny)."""
        thr = np.asarray(thr, np.float64)
        unit = np.maximum(np.abs(thr), TINY)
        with np.errstate(all="ignore"):
            margin = np.abs(q.v - thr) / unit
            on = (np.asarray(q32, np.float64) == thr) & (margin < 2.0 ** -22)
            margin = np.where(on, 0.0, margin)
            gt, ge, lt = (q.v > thr) & ~on, (q.v >= thr) | on, (q.v < thr) & ~on
        entered = np.broadcast_to(entered, margin.shape)
        margin = np.where(np.isnan(q.v), np.inf, margin)          # a NaN compares false with any threshold: nothing to miss
        self.margin[name] = np.where(entered, margin, np.inf)
        self.qerr[name] = np.where(entered & np.isfinite(q.v), q.e / unit, 0.0)
        return gt, ge, lt


def statement(inp):
    """densify_and_prune in float64 -> dict:
    clone, split, keep_orig, keep_clone, keep_child [2,P]: the decisions; margin, qerr: name -> per-row (per-element) arrays;
    counts, src, kind: the layout; val / bound / copied: name -> [Pn, width] float64 values, error bounds and which elements are
    the source row's bits; moments_fresh [Pn]; stats_reset."""
    P = inp["xyz"].shape[0]
    f32q = decide32(inp)["q"]
    C = _Comparisons()
    bounded, rng, lo = _scale_cfg(inp)
    rng, lo = float(rng), float(lo)
    act = (lambda x: e_sigmoid(x) * rng + lo) if bounded else e_exp

    def act_inv(y):
        if not bounded:
            return e_log(y)
        t = (y - lo) / rng                                        # the cancellation in y - lo: e_y / (y - lo) of relative error
        t = t.where(t.v > 0, 0.0)                                 # relu
        return e_log(t / (1.0 - t))                               # e_t / (t (1 - t)); log(0) = -inf where y <= lo

    with np.errstate(all="ignore"):
        p, mr = E(inp["xyz"]), E(inp["max_radii2D"])
        s = act(E(inp["scaling"]))
        smax = e_max3(s)
        dens = e_softplus(E(inp["density"][:, 0]))
        g = E(inp["grad_accum"]) / E(inp["denom"])
        g = g.where(~np.isnan(g.v), 0.0)                          # grads[grads.isnan()] = 0; x / 0 stays +inf
        hot = C.gt("grad", g, f32q["g"], inp["grad_thr"], inp["do_densify"])[1] & inp["do_densify"]
        big = C.gt("scale", smax, f32q["smax"], inp["scale_thr"], inp["do_densify"])[0]
        clone, split = hot & ~big, hot & big
        h = dens.pow2(0.5)
        half = e_log(e_exp(h) - 1.0)                              # e_E / (E - 1): E / (E - 1) ~ 1 / h
        half.v = np.log(np.expm1(h.v))                            # the value itself without the cancellation
        d_orig = half.where(clone, E(inp["density"][:, 0]))
        # the density the prune mask sees: of a cloned row softplus(half) = h up to half's error through softplus' = (E - 1) / E
        soft_e = lambda raw: raw.e / (1.0 + np.exp(-raw.v)) + 4.0 * ulp(h.v)   # noqa: E731
        q_dens = E(h.v, soft_e(half)).where(clone, dens)
        low_d = C.gt("density", q_dens, f32q["dens"], inp["density_min"], ~split)[2]
        b = inp["bbox"].astype(np.float64)
        out_lo = C.gt("box_lo", p, inp["xyz"], b[0])[2]
        out_hi = C.gt("box_hi", p, inp["xyz"], b[1])[0]
        screen_on, scale_on = bool(inp["max_screen"] > 0), bool(inp["max_scale"] > 0)
        big_screen = C.gt("screen", mr, inp["max_radii2D"], inp["max_screen"], screen_on)[0] & screen_on
        big_scale = C.gt("max_scale", smax, f32q["smax"], inp["max_scale"], scale_on & ~split)[0] & scale_on
        pruned = low_d | (out_lo | out_hi).any(axis=1) | big_screen | big_scale
        # children
        q = E(inp["rotation"])
        qq = [E(q.v[:, k]) for k in range(4)]
        n = e_sqrt(qq[0] * qq[0] + qq[1] * qq[1] + qq[2] * qq[2] + qq[3] * qq[3])
        r, x, y, z = (c / n for c in qq)
        R = [[1.0 - (y * y + z * z).pow2(2), (x * y - r * z).pow2(2), (x * z + r * y).pow2(2)],
             [(x * y + r * z).pow2(2), 1.0 - (x * x + z * z).pow2(2), (y * z - r * x).pow2(2)],
             [(x * z - r * y).pow2(2), (y * z + r * x).pow2(2), 1.0 - (x * x + y * y).pow2(2)]]
        s_child = act_inv(s / float(DIV))
        y_child = s.v / float(DIV)
        a_child = np.where(y_child > lo, y_child, lo) if bounded else y_child           # act(act_inv(y))
        d_act = (a_child - lo) * (1.0 - (a_child - lo) / rng) if bounded else a_child   # the activation's derivative there
        q_child_smax = E(a_child.max(axis=1), (np.where(np.isfinite(s_child.v), s_child.e * d_act, 0.0) + 3.0 * ulp(a_child)).max(axis=1))
        q_child_dens = E(h.v, soft_e(half))
        low = C.gt("child_density", q_child_dens, f32q["child_dens"], inp["density_min"], split)[2] | big_screen
        low = low | (C.gt("child_max_scale", q_child_smax, f32q["child_smax"], inp["max_scale"], scale_on & split)[0] & scale_on)
        child_xyz, keep_child = [], []
        for ch in range(2):
            nn = E(inp["normals"][ch])
            v = [E(nn.v[:, k]) * E(s.v[:, k], s.e[:, k]) for k in range(3)]
            rows = [R[j][0] * v[0] + R[j][1] * v[1] + R[j][2] * v[2] + E(p.v[:, j]) for j in range(3)]   # sums of the rotation
            c = E(np.stack([t.v for t in rows], 1), np.stack([t.e for t in rows], 1))
            o_lo = C.gt("child%d_box_lo" % ch, c, f32q["child_xyz"][ch], b[0], split[:, None])[2]
            o_hi = C.gt("child%d_box_hi" % ch, c, f32q["child_xyz"][ch], b[1], split[:, None])[0]
            child_xyz.append(c)
            keep_child.append(split & ~low & ~(o_lo | o_hi).any(axis=1))
    keep = [~split & ~pruned, clone & ~pruned, keep_child[0], keep_child[1]]
    counts = tuple(int(k.sum()) for k in keep)
    src = np.concatenate([np.nonzero(k)[0] for k in keep])
    kind = np.concatenate([np.full(c, kd) for kd, c in enumerate(counts)])
    Pn = len(src)
    child = kind >= CHILD0
    ch = np.where(child, kind - CHILD0, 0)
    val, bound, copied = {}, {}, {}

    def pick(name, computed_rows, computed):
        v = inp[name].astype(np.float64)[src]
        e = np.zeros_like(v)
        m = np.broadcast_to(computed_rows[:, None], v.shape)
        val[name], bound[name], copied[name] = np.where(m, computed.v, v), np.where(m, computed.e, e), ~m

    cx = E(np.stack([c.v for c in child_xyz]), np.stack([c.e for c in child_xyz]))
    pick("xyz", child, E(cx.v[ch, src], cx.e[ch, src]))
    pick("density", child | clone[src], E(half.v[src, None], half.e[src, None]))
    pick("scaling", child, E(s_child.v[src], s_child.e[src]))
    pick("rotation", np.zeros(Pn, bool), E(np.zeros((Pn, 4))))
    for name in NAMES:
        fin = np.isfinite(val[name])
        assert np.isfinite(bound[name][fin]).all(), name          # a finite value has a finite bound
    return dict(P=P, clone=clone, split=split, keep_orig=keep[0], keep_clone=keep[1], keep_child=np.stack(keep[2:]),
                reasons=dict(density=low_d & ~split, box=(out_lo | out_hi).any(axis=1), screen=big_screen, max_scale=big_scale & ~split),
                margin=C.margin, qerr=C.qerr, counts=counts, src=src, kind=kind, val=val, bound=bound, copied=copied,
                moments_fresh=kind != ORIGINAL, stats_reset=inp["do_densify"],
                t_child=((y_child - lo) / rng if bounded else None))


# ------------------------------------------------------------------------------------------------ the comparator
def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def check(result, inp, ref, ratios=None):
    """``result`` (the dict of ``restate32`` / ``result_of``) is densify_and_prune of ``inp`` as ``ref = statement(inp)`` has it:
    counts and layout, the source of every row, copied fields bit for bit, fresh moments +0.0, computed values within their
    bounds with -inf and NaN where the statement has them.  No row is left out.  ``ratios``: a dict that receives the worst
    error / bound per value family."""
    Pn = sum(ref["counts"])
    if result["counts"] is None:      # a statement that reports no counts: the number of rows, the segments through the sources
        assert result["xyz"].shape[0] == Pn, (result["xyz"].shape[0], ref["counts"])
    else:
        assert tuple(result["counts"]) == ref["counts"], (tuple(result["counts"]), ref["counts"])
    for n in NAMES:
        assert result[n].shape == (Pn, WIDTHS[n]) and result[n].dtype == F32, (n, result[n].shape, result[n].dtype)
    # the source of every row, from its rotation row (every kind copies it bit for bit; the rows are pairwise distinct)
    key = lambda rows: [r.tobytes() for r in _bits(rows)]         # noqa: E731
    index = {k: i for i, k in enumerate(key(inp["rotation"]))}
    assert len(index) == inp["rotation"].shape[0], "the input rotations are not pairwise distinct"
    got_src = np.array([index.get(k, -1) for k in key(result["rotation"])])
    bad = np.nonzero(got_src != ref["src"])[0]
    assert not len(bad), "%d rows from the wrong source, first: row %d (%s) from %d, not %d" % (
        len(bad), bad[0], ("original", "clone", "child 0", "child 1")[ref["kind"][bad[0]]], got_src[bad[0]], ref["src"][bad[0]])
    src = ref["src"]
    for n in NAMES:
        got, cp = result[n], ref["copied"][n]
        same = _bits(got) == _bits(inp[n][src])
        assert same[cp].all(), "%s: %d copied elements are not the source's bits" % (n, int((~same[cp]).sum()))
        want, tol = ref["val"][n], ref["bound"][n]
        fin = np.isfinite(want) & ~cp
        odd = ~np.isfinite(want) & ~cp                            # -inf and NaN fall exactly where the statement has them
        g64 = got.astype(np.float64)
        assert np.array_equal(np.isnan(g64[odd]), np.isnan(want[odd])) and np.array_equal(g64[odd][~np.isnan(want[odd])],
                                                                                           want[odd][~np.isnan(want[odd])]), \
            "%s: -inf / NaN not where the statement has them" % n
        assert np.isfinite(g64[fin]).all(), "%s: non-finite where the statement is finite" % n
        with np.errstate(invalid="ignore"):
            err = np.abs(g64 - want)
        over = fin & (err > tol)
        assert not over.any(), "%s: %d values out of their bound, worst error / bound %.3g" % (
            n, int(over.sum()), float((err[over] / tol[over]).max()))
        if ratios is not None and fin.any():
            ratios[n] = max(ratios.get(n, 0.0), float((err[fin] / tol[fin]).max()))
    if inp["moments"] is None:
        assert result["moments"] is None
    else:
        fresh = ref["moments_fresh"]
        for n in NAMES:
            for got, given in zip(result["moments"][n], inp["moments"][n]):
                assert got.shape == (Pn, WIDTHS[n]) and got.dtype == F32
                assert np.array_equal(_bits(got)[~fresh], _bits(given[src])[~fresh]), "moments of %s: an original's differ" % n
                assert not _bits(got)[fresh].any(), "moments of %s: a fresh row's are not +0.0" % n
    assert np.array_equal(_bits(result["max_radii2D"]), _bits(inp["max_radii2D"][src])), "max_radii2D is not inherited"
    for k in ("grad_accum", "denom"):
        got = _bits(np.asarray(result[k]).reshape(-1))
        if ref["stats_reset"]:
            assert not got.any(), k + " is not reset to +0.0"
        else:
            assert np.array_equal(got, _bits(inp[k][src])), k + " is not carried over"


# ------------------------------------------------------------------------------------------------ the statistics of a view
def stats_statement(radii, g2d, max_radii2D, grad_accum, denom):
    """add_densification_stats (gaussian_model.py:552-556, train.py:151-154) of one view -> (visible, max_radii2D, grad_accum as E,
    denom): max and count exact in float32, the accumulated norm in float64 with its bound in densify_stats_view's order."""
    vis = np.asarray(radii) > 0
    mr = np.where(vis, np.maximum(max_radii2D, np.asarray(radii).astype(F32)), max_radii2D).astype(F32)
    dn = np.where(vis, denom + F32(1), denom).astype(F32)
    gx, gy = E(g2d[:, 0]), E(g2d[:, 1])
    acc = E(grad_accum) + e_sqrt(gx * gx + gy * gy)               # grad_scale = 1: the product with it is exact
    return vis, mr, acc.where(vis, E(grad_accum)), dn


# ------------------------------------------------------------------------------------------------ the edge scene
BBOX = np.array([[-1.0, -0.75, -0.5], [1.0, 0.5, 0.75]], F32)       # every face its own value
GRAD_THR = F32(2.0 ** -14)
MAX_SCREEN = F32(48.0)
BOUNDARIES = (0, 255, 256, 4095, 4096, 8191, 8192)                  # rows on each side of a workgroup / scan-tile (4096) boundary


def _on_scale(scale_bound):
    """The largest scale of a row whose largest raw scaling is 0, formed in float32 as the kernel forms it: expf(0) = 1, or
    sigmoid(0) * range + lo = 0.5f * (hi - lo) + lo."""
    if scale_bound is None:
        return F32(1.0)
    lo, hi = F32(scale_bound[0]), F32(scale_bound[1])
    return F32(F32(0.5) * F32(hi - lo) + lo)


def edge_case(P, scale_bound, seed, prune_only=False, moments=True):
    """A cloud of P rows in which every branch of densify_and_prune is taken and nothing but the planted rows is near a threshold
    -> (inputs, planted): planted maps a label to (row, expected (clone, split, keep_orig, keep_clone, keep_child0,
    keep_child1)).  Rows on both sides of every launch boundary (BOUNDARIES, P - 1) survive, with clones and splits among them.
    prune_only: do_densify off and the density threshold at 21, above the softplus threshold, where a density is its raw bits.
    From 128 rows on every planted row is there; below, only the boundary rows."""
    rng = np.random.default_rng(seed)
    S0 = _on_scale(scale_bound)
    density_min = F32(21.0) if prune_only else F32(2.0 ** -10)
    # modes: 0 free; forced rows that survive: 1 hot and small (cloned), 2 hot and large (split, both children stay), 3 cold
    mode = np.zeros(P, np.int64)
    edges = sorted({b for b in BOUNDARIES + (P - 1,) if 0 <= b < P})
    for k, b in enumerate(edges):
        mode[b] = (2, 1, 3)[k % 3]
    if prune_only:
        mode[mode == 2] = 1                                       # a large row is above max_scale: it would be pruned

    def draw(idx):
        n = len(idx)
        m = mode[idx]
        forced = (m > 0)[:, None]
        span = (BBOX[1] - BBOX[0]).astype(np.float64)
        xyz = np.where(forced, rng.uniform(-0.1, 0.1, (n, 3)), BBOX[0] + span * rng.uniform(-0.02, 1.02, (n, 3)))
        if prune_only:
            dens = np.where(forced[:, 0] | (rng.random(n) < 0.5), rng.uniform(22.0, 30.0, n), rng.uniform(-12.0, 3.0, n))
        else:
            dens = np.where(forced[:, 0], rng.uniform(0.0, 3.0, n), rng.uniform(-12.0, 3.0, n))
        free_scal = rng.uniform(-7.0, 5.0, (n, 3)) if scale_bound is not None else rng.uniform(np.log(0.02), np.log(2.5), (n, 3))
        small = rng.uniform(-3.0, -0.5, (n, 3))
        large = small.copy()
        large[np.arange(n), rng.integers(0, 3, n)] = rng.uniform(0.1, 0.4, n)
        scal = np.where(m[:, None] == 0, free_scal, np.where(m[:, None] == 2, large, small))
        rot = rng.normal(size=(n, 4))
        mr = np.where(forced[:, 0], rng.uniform(0.0, 40.0, n), rng.uniform(0.0, 54.0, n))
        dn = rng.integers(0, 9, n).astype(np.float64)
        ga = rng.uniform(0.0, 4.0, n) * float(GRAD_THR) * np.maximum(dn, rng.integers(0, 2, n))   # 0 / 0 and x / 0 among them
        hot, cold = (m == 1) | (m == 2), m == 3
        dn = np.where(hot | cold, 2.0, dn)
        ga = np.where(hot, 8.0 * float(GRAD_THR), np.where(cold, 0.0, ga))
        nrm = np.where(forced[None], rng.uniform(-0.1, 0.1, (2, n, 3)), rng.normal(size=(2, n, 3)))
        return dict(xyz=xyz, density=dens[:, None], scaling=scal, rotation=rot, max_radii2D=mr, grad_accum=ga, denom=dn, normals=nrm)

    a = {k: v.astype(F32) for k, v in draw(np.arange(P)).items()}
    # ---- planted rows: a neutral row (inside, dense, small, cold) with one thing on a threshold
    planted, spec = {}, []
    up = lambda x: np.nextafter(F32(x), F32(np.inf))              # noqa: E731
    down = lambda x: np.nextafter(F32(x), F32(-np.inf))           # noqa: E731
    HOT = dict(grad_accum=F32(8) * GRAD_THR, denom=F32(2))
    LARGE = dict(scaling=(0.3, -1.0, -0.5))
    KEEP, GONE, CLONED, SPLIT = (0, 0, 1, 0, 0, 0), (0, 0, 0, 0, 0, 0), (1, 0, 1, 1, 0, 0), (0, 1, 0, 0, 1, 1)
    ON, OFF = (0.0, -1.0, -2.0), (2.0 ** -19, -1.0, -2.0)       # largest scale on S0; 8 ulp or more above it (2 ulp are the
    UNDER = (-2.0 ** -19, -1.0, -2.0)                             # activation's own)
    if not prune_only:
        spec += [("grad on", dict(grad_accum=GRAD_THR * F32(4), denom=F32(4)), CLONED),
                 ("grad below", dict(grad_accum=down(GRAD_THR * F32(4)), denom=F32(4)), KEEP),
                 ("grad 0/0", dict(grad_accum=F32(0), denom=F32(0)), KEEP),
                 ("grad x/0", dict(grad_accum=F32(2.0 ** -20), denom=F32(0)), CLONED),
                 ("scale on, hot", dict(HOT, scaling=ON), CLONED), ("scale above, hot", dict(HOT, scaling=OFF), SPLIT),
                 ("scale under, hot", dict(HOT, scaling=UNDER), CLONED),
                 ("halved density under", dict(HOT, density=F32(np.log(np.expm1(1.5 * float(density_min))))), (1, 0, 0, 0, 0, 0)),
                 ("split at a face", dict(HOT, **LARGE, xyz=(BBOX[1, 0], 0.0, 0.0), rotation=(2.0, 0.0, 0.0, 0.0),
                                          normals=((-1.0, 0.1, 0.1), (1.0, 0.1, 0.1))), (0, 1, 0, 0, 1, 0)),
                 ("screen on, split", dict(HOT, **LARGE, max_radii2D=MAX_SCREEN), SPLIT),
                 ("screen above, split", dict(HOT, **LARGE, max_radii2D=up(MAX_SCREEN)), (0, 1, 0, 0, 0, 0)),
                 ("quaternion 1e-3", dict(HOT, **LARGE, rotation=rng.normal(size=4) * 1e-3), SPLIT),
                 ("quaternion 1e3", dict(HOT, **LARGE, rotation=rng.normal(size=4) * 1e3), SPLIT),
                 ("quaternion zero", dict(HOT, **LARGE, rotation=(0.0, 0.0, 0.0, 0.0)), SPLIT)]   # NaN children: kept
        if scale_bound is not None:                               # an axis whose scale / 1.6 is far under lo: raw scaling -inf
            spec += [("shrunk child %d" % k, dict(HOT, scaling=np.roll((0.3, -15.0, 0.5), k)), SPLIT) for k in range(2)]
    else:
        spec += [("density on", dict(density=F32(21.0)), KEEP), ("density below", dict(density=down(21.0)), GONE),
                 ("hot, no densification", dict(HOT), KEEP)]
    spec += [("scale on, cold", dict(scaling=ON), KEEP), ("scale above, cold", dict(scaling=OFF), GONE),
             ("screen on", dict(max_radii2D=MAX_SCREEN), KEEP), ("screen above", dict(max_radii2D=up(MAX_SCREEN)), GONE),
             ("nan coordinate", dict(xyz=(0.0, np.nan, 0.0)), KEEP)]
    for ax in range(3):
        for side, step in ((0, down), (1, up)):
            on = np.zeros(3, F32)
            on[ax] = BBOX[side, ax]
            off = on.copy()
            off[ax] = step(on[ax])
            spec += [("face %d%d on" % (ax, side), dict(xyz=on), KEEP), ("face %d%d outside" % (ax, side), dict(xyz=off), GONE)]
    is_planted = np.zeros(P, bool)
    if P >= 128:
        free = np.nonzero(mode == 0)[0]
        rows = rng.choice(free, len(spec), replace=False)
        neutral = dict(xyz=(0.0, 0.0, 0.0), density=F32(25.0 if prune_only else 1.0), scaling=(-1.0, -2.0, -1.5), max_radii2D=F32(1.0),
                       grad_accum=F32(0), denom=F32(1))
        for row, (label, over, expect) in zip(rows, spec):
            a["normals"][:, row] = rng.uniform(-0.1, 0.1, (2, 3)).astype(F32)
            for k, v in dict(neutral, **over).items():
                if k == "normals":
                    a[k][:, row] = np.asarray(v, F32)
                else:
                    a[k][row] = np.asarray(v, F32)
            planted[label] = (int(row), expect)
            is_planted[row] = True

    def inputs():
        mom = None
        if moments:
            r2 = np.random.default_rng(seed + 1)
            mom = {n: (r2.normal(size=(P, WIDTHS[n])).astype(F32), r2.random((P, WIDTHS[n])).astype(F32)) for n in NAMES}
        return make_inputs({n: a[n] for n in NAMES}, mom, a["max_radii2D"], a["grad_accum"], a["denom"], a["normals"], GRAD_THR, S0,
                           density_min, BBOX, scale_bound, not prune_only, MAX_SCREEN, S0)

    # ---- redraw, never skip: every row that is not planted keeps every margin
    for _round in range(200):
        inp = inputs()
        ref = statement(inp)
        near = np.zeros(P, bool)
        for k, m in ref["margin"].items():
            miss = (m <= MARGIN) | (m <= 4.0 * ref["qerr"][k])
            near |= miss.reshape(P, -1).any(axis=1)
        if ref["t_child"] is not None:
            near |= ref["split"] & (ref["t_child"] <= 1e-3).any(axis=1)
        _u, first = np.unique(inp["rotation"], axis=0, return_index=True)
        dup = np.ones(P, bool)
        dup[first] = False
        near |= dup
        forced_ok = np.where(mode == 2, ref["keep_child"].all(axis=0), np.where(mode == 1, ref["keep_clone"] | prune_only, True))
        near |= (mode > 0) & ~(forced_ok & (ref["keep_orig"] | ref["split"]))
        near &= ~is_planted
        if not near.any():
            break
        idx = np.nonzero(near)[0]
        for k, v in draw(idx).items():
            if k == "normals":
                a[k][:, idx] = v.astype(F32)
            else:
                a[k][idx] = v.astype(F32)
    else:
        raise AssertionError("edge_case: rows still near a threshold after 200 redraws")
    # ---- what the scene promises, asserted
    f32 = decide32(inp)
    got = np.stack([ref["clone"], ref["split"], ref["keep_orig"], ref["keep_clone"], ref["keep_child"][0], ref["keep_child"][1]], 1)
    for label, (row, expect) in planted.items():
        assert tuple(int(x) for x in got[row]) == expect, (label, row, got[row], expect)
    if planted:
        on = lambda label: planted[label][0]                      # noqa: E731
        assert all(f32["q"]["smax"][on(k)] == S0 for k in planted if k.startswith("scale on"))       # exact in float32
        assert all(f32["q"]["smax"][on(k)] > S0 for k in planted if k.startswith("scale above"))
        if not prune_only:
            assert f32["q"]["g"][on("grad on")] == GRAD_THR and f32["q"]["g"][on("grad below")] < GRAD_THR
            assert np.isposinf(f32["q"]["g"][on("grad x/0")]) and f32["q"]["g"][on("grad 0/0")] == 0
            assert ref["margin"]["grad"][on("grad on")] == 0 and ref["margin"]["scale"][on("scale on, hot")] == 0
            kids = ref["val"]["xyz"][(ref["src"] == on("quaternion zero")) & (ref["kind"] >= CHILD0)]
            assert kids.shape == (2, 3) and np.isnan(kids).all()
            if scale_bound is not None:
                kid = ref["val"]["scaling"][(ref["src"] == on("shrunk child 0")) & (ref["kind"] == CHILD0)][0]
                assert np.isneginf(kid).sum() == 1 and np.isfinite(kid).sum() == 2
        else:
            assert f32["q"]["dens"][on("density on")] == density_min and ref["margin"]["density"][on("density on")] == 0
            assert f32["q"]["dens"][on("density below")] == down(21.0)
    if P >= 255:
        assert all(c > 0 for c in ref["counts"][:1 if prune_only else 4]), ref["counts"]
        assert all(int(v.sum()) > 0 for v in ref["reasons"].values()), {k: int(v.sum()) for k, v in ref["reasons"].items()}
        assert prune_only or ref["keep_child"].sum() < 2 * ref["split"].sum()   # and children are pruned too
        at = np.array(edges)
        assert (ref["keep_orig"][at] | ref["keep_child"][:, at].all(axis=0)).all()
        assert prune_only or (ref["split"][at].any() and ref["clone"][at].any())
    return inp, planted


def result_of(new_params, new_moments, max_radii2D, grad_accum, denom, counts):
    """What densify.densify_and_prune returned (anything ``np.asarray`` takes, already on the host) as ``check``'s dict."""
    out = {n: np.ascontiguousarray(np.asarray(new_params[n], F32)) for n in NAMES}
    out["moments"] = None if new_moments is None else {n: tuple(np.ascontiguousarray(np.asarray(t, F32)) for t in new_moments[n])
                                                        for n in NAMES}
    for k, t in (("max_radii2D", max_radii2D), ("grad_accum", grad_accum), ("denom", denom)):
        out[k] = np.ascontiguousarray(np.asarray(t, F32)).reshape(-1)
    out["counts"] = None if counts is None else tuple(int(c) for c in counts)
    return out


def stats_case(P, seed):
    """One view for r2_densify_stats: radii with 0 and negative values, gradients from 1e-30 to 1e20 (gx * gx underflows and
    overflows float32), a NaN gradient on a visible and on an invisible row -> (radii, g2d, max_radii2D, grad_accum, denom)."""
    rng = np.random.default_rng(seed)
    radii = rng.integers(-3, 40, P).astype(np.int32)
    radii[rng.random(P) < 0.3] = 0
    g2d = (10.0 ** rng.uniform(-30.0, 20.0, (P, 3)) * rng.choice([-1.0, 1.0], (P, 3))).astype(F32)
    if P >= 255:
        vis, hid = np.nonzero(radii > 0)[0], np.nonzero(radii <= 0)[0]
        g2d[vis[0], 0] = g2d[hid[0], 1] = np.nan
        g2d[vis[1]] = (1e-30, 1e-30, 1.0)
        g2d[vis[2]] = (1e18, -1e18, 1.0)
        g2d[vis[3]] = (1e20, 1e-30, 1.0)
    return (radii, g2d, rng.uniform(0.0, 60.0, P).astype(F32), rng.uniform(0.0, 1.0, P).astype(F32),
            rng.integers(0, 5, P).astype(F32))


def check_stats(result, case):
    """``result`` = (max_radii2D, grad_accum, denom) after r2_densify_stats on ``case`` (stats_case's tuple): invisible rows keep
    their bits, the maximum and the count are exact, the accumulated norm is within its bound of float64, with NaN and inf where
    float32 has them."""
    radii, g2d, mr, ga, dn = case
    vis, mr_ref, acc, dn_ref = stats_statement(radii, g2d, mr, ga, dn)
    got_mr, got_ga, got_dn = (np.ascontiguousarray(np.asarray(t, F32)).reshape(-1) for t in result)
    for got, given in ((got_mr, mr), (got_ga, ga), (got_dn, dn)):
        assert np.array_equal(_bits(got)[~vis], _bits(given)[~vis]), "an invisible row was touched"
    assert np.array_equal(_bits(got_mr), _bits(mr_ref)) and np.array_equal(_bits(got_dn), _bits(dn_ref))
    fin = np.isfinite(acc.v) & vis
    g64 = got_ga.astype(np.float64)
    assert np.array_equal(np.isnan(g64), np.isnan(acc.v)) and np.array_equal(np.isposinf(g64), np.isposinf(acc.v))
    err = np.abs(g64[fin] - acc.v[fin])
    assert (err <= acc.e[fin]).all(), "grad_accum: worst error / bound %.3g" % float((err / acc.e[fin]).max())
