"""Float64 restatement of the Siddon forward projector (csrc/projector_siddon.hip, include/r2hip.h:
r2_project_volume_siddon), a dense system matrix for tiny systems, and the per-pixel float32 error bound the kernel is
checked against.  Host only; the product never imports this file.

The restatement does not walk the grid.  For one ray it clips the line to the volume [-1/2, n_a - 1/2]^3 in float64, merges
the sorted plane crossings t = (m - 1/2 - S_a) / D_a of the three axes that fall inside the clipped chord, and takes the cell
of each segment from the segment's midpoint (floor(q + 1/2)): value = |D (.) dVoxel| sum_seg (t_next - t_cur) vol[cell].  It
evaluates this from the float32 ray parameters the kernel is given, so that the only differences left are the kernel's
float32 roundings and its orderings of nearly equal crossings.

Bound (u = 2^-24, the float32 unit roundoff; first order in u; ``SAFETY`` covers the dropped higher-order terms).  For one
pixel with ray point P = p00 + c pu + r pv, start S and direction D (cone: S = a, D = P - S; parallel: S = P, D = a):

* P: two products and two sums, |dP_a| <= 4 u (|p00_a| + c |pu_a| + r |pv_a|); cone: |dD_a| <= |dP_a| + u |D_a|;
  parallel: |dS_a| = |dP_a| (tests/projector_ref.py states the same).
* plane_t(m) = ((m - 1/2) - s) * rd with rd = 1 / d: m - 1/2 is exact, then a rounded subtraction, the rounded reciprocal
  and a rounded product, 3 u relative, plus the inputs' errors: E(t) = |t| (3 u + |dD_a| / |D_a|) + |dS_a| / |D_a| for a
  crossing of axis a at t.  The clip points are such crossings (E0 at t0, E1 at t1: the largest E among the axes that
  are within their E of deciding the max or min; a cone's t0 = 0 is exact).  First order in |dD_a| / |D_a|: a direction
  component within twice its own error (a ray nearly parallel to a family of planes) gets E = infinity for the crossings
  it makes inside the chord, and takes no part in the clip when its volume faces lie beyond twice the chord's range of t
  for every direction within the error.
* endpoints: the kernel uses one float per crossing, as the end of a segment and the start of the next, so the sum
  telescopes: sum_seg v_seg (dt_next - dt_cur) = - sum_crossings dt_c (v_after - v_before) + ends, bounded by
  sum_c E(t_c) |v_after - v_before| + E0 |v_first| + E1 |v_last|.  A constant volume leaves only the ends.
* segments: each (t_next - t_cur) * v is a rounded difference and a rounded product, and the n_seg terms are summed in
  order: (n_seg + 2) u sum_seg |(t_next - t_cur) v|.
* near ties: a run of consecutive crossings (the clip points included) whose gaps are each within the sum of their two E
  may come in any order in float32, the tie rule x, y, z included.  Whatever the order, the cells visited inside the run lie
  in the box between the cell before the run and the cell after it, and the time spent in them is at most
  G = (t_last - t_first) + sum E over the run, in the restatement as in the kernel; subtracting the box's mid-range value
  from both leaves 2 G * (max - min of vol over that box) / 2 on each side: 2 G range(box) in all.  That is the tie gap (plus
  its uncertainty) times the local voxel difference.
* a ray that only grazes the volume (|t1 - t0| <= E0 + E1) may hit in one arithmetic and miss in the other: the chord is
  then at most E0 + E1 long, (E0 + E1) max |vol|.  An axis the ray does not move along (D_a = 0) decides its slab from S_a
  alone: when S_a is within |dS_a| of a slab boundary the kernel may sit in the neighbouring slab (or outside the volume)
  for the whole chord, 2 (t1 - t0) max |vol|.  The same holds for a direction component within twice its own error of 0
  (the centre column of a cone view that looks along an axis: the kernel's own d_a may be 0 or of either sign): over the
  chord the position on that axis moves by less than its error |dS_a| + |t| |dD_a| + u |q_a|, and when a slab boundary
  lies within that error of it the kernel may run along the other side of the boundary for the whole chord.
* the factor |D (.) dVoxel|: 6 u relative plus sum_a dVoxel_a |dD_a| / |D_world|, and u for the final product.

No pixel is exempt: every term above is part of every pixel's bound, most of them zero for most pixels.
"""
import numpy as np

U = 2.0 ** -24
SAFETY = 2.0


def _ray_geometry(ray12, cone, pixels):
    """S, D and their float32 error bounds eS, eD for pixels [N, 3] (view, row, col) of float32 ray parameters [V, 12]."""
    R12 = np.asarray(ray12, np.float32).astype(np.float64)
    pv = R12[pixels[:, 0]]
    r = pixels[:, 1].astype(np.float64)[:, None]
    c = pixels[:, 2].astype(np.float64)[:, None]
    P = pv[:, 3:6] + c * pv[:, 6:9] + r * pv[:, 9:12]
    eP = 4 * U * (np.abs(pv[:, 3:6]) + c * np.abs(pv[:, 6:9]) + r * np.abs(pv[:, 9:12]))
    if cone:
        S, D = pv[:, 0:3].copy(), P - pv[:, 0:3]
        eS, eD = np.zeros_like(eP), eP + U * np.abs(D)
    else:
        S, D = P, pv[:, 0:3].copy()
        eS, eD = eP, np.zeros_like(eP)
    return S, D, eS, eD


def trace(S, D, n, cone, eS=None, eD=None):
    """One ray against the grid of n = (nx, ny, nz) cells.  -> dict(hit, t0, t1, edges [n_seg + 1] (t0, the crossings, t1),
    E [n_seg + 1] (their float32 error bounds), cells [n_seg, 3], flat_edge: S on a flat axis is within eS of a slab
    boundary, inside: the flat axes hold the ray)."""
    S, D = np.asarray(S, np.float64), np.asarray(D, np.float64)
    n = np.asarray(n, np.int64)
    eS = np.zeros(3) if eS is None else eS
    eD = np.zeros(3) if eD is None else eD
    lo, hi = np.full(3, -np.inf), np.full(3, np.inf)
    e_of = []
    inside, flat_edge = True, False
    for a in range(3):
        if D[a] == 0.0:
            inside &= bool(-0.5 <= S[a] < n[a] - 0.5)
            frac = S[a] + 0.5 - np.floor(S[a] + 0.5)
            flat_edge |= bool(min(frac, 1.0 - frac) <= eS[a]) and -0.5 - eS[a] <= S[a] <= n[a] - 0.5 + eS[a]
            e_of.append(None)
            continue
        # first order in dD / D; a direction component within twice its own error has no usable bound
        rel = 3 * U + eD[a] / abs(D[a]) if 2 * eD[a] < abs(D[a]) else np.inf
        e_of.append((rel, eS[a] / abs(D[a])))
        ta, tb = (-0.5 - S[a]) / D[a], (n[a] - 0.5 - S[a]) / D[a]
        lo[a], hi[a] = min(ta, tb), max(ta, tb)
    t0, t1 = lo.max(), hi.min()
    if cone:
        t0 = max(t0, 0.0)

    def err(a, t):
        return (abs(t) * e_of[a][0] if t != 0 else 0.0) + e_of[a][1]

    # an axis whose volume faces the kernel's ray cannot reach within twice the chord's range of t, whatever the rounding of
    # its direction (a ray nearly parallel to them), does not decide a clip point
    reach = 2.0 * max(abs(t0), abs(t1))
    reach = reach if np.isfinite(reach) else np.inf

    def decides(a):
        near = min(abs(-0.5 - S[a]), abs(n[a] - 0.5 - S[a])) - eS[a]
        return e_of[a] is not None and near <= (abs(D[a]) + eD[a]) * reach

    E0 = max([err(a, lo[a]) for a in range(3) if decides(a) and lo[a] + err(a, lo[a]) >= t0], default=0.0)
    E1 = max([err(a, hi[a]) for a in range(3) if decides(a) and hi[a] - err(a, hi[a]) <= t1], default=0.0)
    moves = any(e is not None for e in e_of)
    # an axis whose direction component is within twice its own error of 0 is flat or nearly so for the kernel as well: the
    # ray keeps to one slab over the chord, and which one is open when a slab boundary lies within the position's error
    if np.isfinite(t0) and np.isfinite(t1) and t1 > t0:
        for a in range(3):
            if D[a] == 0.0 or e_of[a][0] != np.inf:
                continue
            qa, qb = S[a] + t0 * D[a], S[a] + t1 * D[a]
            w = eS[a] + max(abs(t0), abs(t1)) * eD[a] + U * max(abs(qa), abs(qb))
            q_lo, q_hi = max(min(qa, qb) - w, -0.5 - w), min(max(qa, qb) + w, n[a] - 0.5 + w)
            flat_edge |= bool(q_lo <= q_hi and np.floor(q_lo + 0.5) != np.floor(q_hi + 0.5)) or \
                bool(q_lo <= -0.5 <= q_hi) or bool(q_lo <= n[a] - 0.5 <= q_hi)
    out = dict(hit=bool(inside and moves and t1 > t0), inside=inside, moves=moves, t0=t0, t1=t1, E0=E0, E1=E1,
               flat_edge=flat_edge)
    if not out["hit"]:
        return out
    ts, es, axes = [], [], []
    for a in range(3):
        if e_of[a] is None:
            continue
        t = (np.arange(n[a] + 1) - 0.5 - S[a]) / D[a]
        t = t[(t > t0) & (t < t1)]
        ts.append(t)
        es.append(np.where(t != 0, np.abs(t) * e_of[a][0], 0.0) + e_of[a][1])
        axes.append(np.full(len(t), a))
    ts, es, axes = np.concatenate(ts), np.concatenate(es), np.concatenate(axes)
    order = np.lexsort((axes, ts))
    edges = np.concatenate([[t0], ts[order], [t1]])
    E = np.concatenate([[E0], es[order], [E1]])
    mid = 0.5 * (edges[:-1] + edges[1:])
    cells = np.floor(S[None, :] + mid[:, None] * D[None, :] + 0.5).astype(np.int64)
    cells = np.clip(cells, 0, n - 1)
    out.update(edges=edges, E=E, cells=cells)
    return out


def project(vol, ray12, cone, dVoxel, H, W, pixels=None):
    """Restatement on float32 ray parameters ray12 [V, 12].  pixels: optional [N, 3] (view, row, col) subset.
    -> dict(value, bound, chord (the clipped chord's world length, 0 for a miss), n_seg, hit, pixels) flattened over the
    pixels (row-major [V,H,W] when pixels is None)."""
    vol = np.asarray(vol, np.float64)
    n = np.array(vol.shape)
    V = len(ray12)
    if pixels is None:
        vv, rr, cc = np.meshgrid(np.arange(V), np.arange(H), np.arange(W), indexing="ij")
        pixels = np.stack([vv.ravel(), rr.ravel(), cc.ravel()], 1)
    pixels = np.asarray(pixels)
    S, D, eS, eD = _ray_geometry(ray12, cone, pixels)
    dv = np.asarray(dVoxel, np.float64)
    vmax = float(np.abs(vol).max(initial=0.0))
    N = len(pixels)
    value, bound, chord = np.zeros(N), np.zeros(N), np.zeros(N)
    n_seg, hit = np.zeros(N, np.int64), np.zeros(N, bool)
    for p in range(N):
        tr = trace(S[p], D[p], n, cone, eS[p], eD[p])
        wlen = float(np.sqrt(((D[p] * dv) ** 2).sum()))
        e_wlen_rel = 6 * U + (float(np.sqrt(((eD[p] * dv) ** 2).sum())) / wlen if wlen > 0 else 0.0)
        span = tr["t1"] - tr["t0"]
        b = 0.0
        if tr["inside"] and tr["moves"] and np.isfinite(span) and abs(span) <= tr["E0"] + tr["E1"]:
            b += (tr["E0"] + tr["E1"]) * vmax
        if tr["flat_edge"] and tr["moves"] and np.isfinite(span) and span > 0:
            b += 2.0 * span * vmax
        if tr["hit"]:
            edges, E, cells = tr["edges"], tr["E"], tr["cells"]
            v = vol[cells[:, 0], cells[:, 1], cells[:, 2]]
            seg = np.diff(edges)
            acc = float((seg * v).sum())
            value[p] = wlen * acc
            chord[p] = wlen * span
            n_seg[p] = len(seg)
            hit[p] = True
            b += float((E[1:-1] * np.abs(np.diff(v))).sum()) + E[0] * abs(v[0]) + E[-1] * abs(v[-1])
            b += (len(seg) + 2) * U * float(np.abs(seg * v).sum())
            # runs of near ties among the edges (clip points included)
            tied = seg <= E[:-1] + E[1:]
            j = 0
            while j < len(seg):
                if not tied[j]:
                    j += 1
                    continue
                k = j
                while k < len(seg) and tied[k]:
                    k += 1
                # edges j..k form the run; the cell before edge j and the cell after edge k
                before = cells[max(j - 1, 0)]
                after = cells[min(k, len(seg) - 1)]
                lo_c, hi_c = np.minimum(before, after), np.maximum(before, after)
                box = vol[lo_c[0]:hi_c[0] + 1, lo_c[1]:hi_c[1] + 1, lo_c[2]:hi_c[2] + 1]
                G = (edges[k] - edges[j]) + float(E[j:k + 1].sum())
                b += 2.0 * G * float(box.max() - box.min())
                j = k
            b = wlen * b + abs(value[p]) * (e_wlen_rel + U)
        else:
            b = wlen * b
        bound[p] = SAFETY * b
    return dict(value=value, bound=bound, chord=chord, n_seg=n_seg, hit=hit, pixels=pixels)


def dense_A(views, sVoxel, center, nVoxel):
    """-> A [V*H*W, nx*ny*nz] float64 in scene units: row rho holds the world lengths of ray rho inside every voxel, from the
    float32 ray parameters the kernel is given."""
    from r2_gaussian_amd import projector as K
    nVoxel = tuple(int(m) for m in nVoxel)
    cone = views[0].mode == 1
    H, W = views[0].image_height, views[0].image_width
    rays32 = K.ray_params(views, sVoxel, center, nVoxel)
    return dense_A_rays(rays32, cone, np.asarray(sVoxel, np.float64) / np.asarray(nVoxel), nVoxel, H, W)


def dense_A_rays(ray12, cone, dVoxel, nVoxel, H, W):
    n = np.array(nVoxel)
    V = len(ray12)
    vv, rr, cc = np.meshgrid(np.arange(V), np.arange(H), np.arange(W), indexing="ij")
    pixels = np.stack([vv.ravel(), rr.ravel(), cc.ravel()], 1)
    S, D, _, _ = _ray_geometry(ray12, cone, pixels)
    dv = np.asarray(dVoxel, np.float64)
    A = np.zeros((len(pixels), int(np.prod(n))))
    for p in range(len(pixels)):
        tr = trace(S[p], D[p], n, cone)
        if not tr["hit"]:
            continue
        wlen = float(np.sqrt(((D[p] * dv) ** 2).sum()))
        cells = tr["cells"]
        flat = (cells[:, 0] * n[1] + cells[:, 1]) * n[2] + cells[:, 2]
        np.add.at(A[p], flat, wlen * np.diff(tr["edges"]))
    return A


def dense_A_cfg(cfg, angles):
    """A of ``projector.project(..., projection_type="siddon")`` for a raw config (A_scene / scale)."""
    from tests import recon_ref as RR
    views, sV, ctr, scale = RR.scene_geometry(cfg, angles)
    return dense_A(views, sV, ctr, cfg["nVoxel"]) / scale
