"""CPU references of the merge operators (include/r2hip.h: r2_merge_cost, r2_graph_match, r2_merge_count, r2_merge_emit), in
float64 numpy: Runnalls' cost of an edge, the moment-matched Gaussian of a pair, the sequential greedy matching, the
round-limited locally-dominant-edge matching, the validation of a mate array and the merged cloud."""
import numpy as np

# the tests' bounds on a merged row (float outputs against this float64 reference); U = one float32 rounding
U = 2.0 ** -24
MU_REL = 2.0 ** -23        # per component, plus MU_REL * max |mu_a|, |mu_b| absolute
COV_REL = 2.0 ** -20       # Frobenius, relative to the reference covariance: 16 roundings
MASS_REL = 2.0 ** -21      # 8 roundings
COST_REL, COST_ABS = 2.0 ** -23, 1e-9


def quat_to_rot(q):
    """R [.., 3, 3] of the quaternion (r, x, y, z) AS GIVEN (no normalisation): the rasterizer's quat_to_rot."""
    q = np.asarray(q, dtype=np.float64)
    r, x, y, z = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    R = np.empty(q.shape[:-1] + (3, 3))
    R[..., 0, 0] = 1 - 2 * (y * y + z * z); R[..., 0, 1] = 2 * (x * y - r * z); R[..., 0, 2] = 2 * (x * z + r * y)
    R[..., 1, 0] = 2 * (x * y + r * z); R[..., 1, 1] = 1 - 2 * (x * x + z * z); R[..., 1, 2] = 2 * (y * z - r * x)
    R[..., 2, 0] = 2 * (x * z - r * y); R[..., 2, 1] = 2 * (y * z + r * x); R[..., 2, 2] = 1 - 2 * (x * x + y * y)
    return R


def covariance(scaling, rotation):
    """Sigma [.., 3, 3] = R^T diag(s^2) R (cov3d_from_scale_rot with mod = 1)."""
    s = np.asarray(scaling, dtype=np.float64)
    R = quat_to_rot(rotation)
    return np.einsum("...ka,...k,...kb->...ab", R, s * s, R)


def mass(density, scaling):
    d = np.asarray(density, dtype=np.float64).reshape(-1)
    s = np.asarray(scaling, dtype=np.float64).reshape(-1, 3)
    return d * s[:, 0] * s[:, 1] * s[:, 2]


def usable(xyz, density, scaling, rotation):
    """[P] bool: every parameter finite, density > 0, scales > 0."""
    x, d, s, q = (np.asarray(t, dtype=np.float64) for t in (xyz, density, scaling, rotation))
    d = d.reshape(-1)
    fin = np.isfinite(x).all(1) & np.isfinite(d) & np.isfinite(s).all(1) & np.isfinite(q).all(1)
    with np.errstate(invalid="ignore"):
        return fin & (d > 0) & (s > 0).all(1)


def pair_moments(a, b, xyz, density, scaling, rotation):
    """Arrays of pairs a, b -> alpha [n], mu [n, 3], cov [n, 3, 3], mass [n] of the moment-matched Gaussians."""
    x = np.asarray(xyz, dtype=np.float64)
    m = mass(density, scaling)
    cov = covariance(scaling, rotation)
    alpha = m[a] / (m[a] + m[b])
    d = x[a] - x[b]
    al, be = alpha[:, None, None], (1 - alpha)[:, None, None]
    cab = al * cov[a] + be * cov[b] + (al * be) * d[:, :, None] * d[:, None, :]
    mu = alpha[:, None] * x[a] + (1 - alpha)[:, None] * x[b]
    return alpha, mu, cab, m[a] + m[b]


def edge_costs(idx, xyz, density, scaling, rotation, max_trace=0.0):
    """cost [P, K] float64: max(0, 1/2 [log det S_ab - alpha log det S_a - (1 - alpha) log det S_b]) with a = min(i, j),
    b = max(i, j); +inf on invalid and self edges, unusable ends, a non-finite result, and trace S_ab > max_trace > 0."""
    idx = np.asarray(idx)
    P, K = idx.shape
    out = np.full((P, K), np.inf)
    if P == 0:
        return out
    ok = usable(xyz, density, scaling, rotation)
    i = np.repeat(np.arange(P), K).reshape(P, K)
    valid = (idx >= 0) & (idx < P) & (idx != i)
    j = np.where(valid, idx, 0)
    valid &= ok[i] & ok[j]
    a, b = np.minimum(i, j)[valid], np.maximum(i, j)[valid]
    if a.size == 0:
        return out
    with np.errstate(all="ignore"):
        alpha, _mu, cab, _m = pair_moments(a, b, xyz, density, scaling, rotation)
        cov = covariance(scaling, rotation)
        sa, la = np.linalg.slogdet(cov[a])
        sb, lb = np.linalg.slogdet(cov[b])
        sab, lab = np.linalg.slogdet(cab)
        c = 0.5 * (lab - alpha * la - (1 - alpha) * lb)
        c = np.where((sa > 0) & (sb > 0) & (sab > 0) & np.isfinite(c), np.maximum(c, 0.0), np.inf)
        if max_trace > 0:
            c = np.where(np.trace(cab, axis1=1, axis2=2) > max_trace, np.inf, c)
    out[valid] = c
    return out


def canonical_quat(R):
    """The unit quaternion (r, x, y, z) of a rotation matrix R (quat_to_rot's inverse) with r >= 0, the first non-zero component
    positive when r = 0."""
    f = np.array([1 + R[0, 0] + R[1, 1] + R[2, 2], 1 + R[0, 0] - R[1, 1] - R[2, 2], 1 - R[0, 0] + R[1, 1] - R[2, 2],
                  1 - R[0, 0] - R[1, 1] + R[2, 2]])
    k = int(np.argmax(f))
    h = 0.5 * np.sqrt(f[k])
    q = np.empty(4)
    if k == 0:
        q[:] = h, (R[2, 1] - R[1, 2]) / (4 * h), (R[0, 2] - R[2, 0]) / (4 * h), (R[1, 0] - R[0, 1]) / (4 * h)
    elif k == 1:
        q[:] = (R[2, 1] - R[1, 2]) / (4 * h), h, (R[0, 1] + R[1, 0]) / (4 * h), (R[0, 2] + R[2, 0]) / (4 * h)
    elif k == 2:
        q[:] = (R[0, 2] - R[2, 0]) / (4 * h), (R[0, 1] + R[1, 0]) / (4 * h), h, (R[1, 2] + R[2, 1]) / (4 * h)
    else:
        q[:] = (R[1, 0] - R[0, 1]) / (4 * h), (R[0, 2] + R[2, 0]) / (4 * h), (R[1, 2] + R[2, 1]) / (4 * h), h
    q /= np.linalg.norm(q)
    lead = q[np.flatnonzero(q)[0]]
    return -q if lead < 0 else q


def merged_row(cov, total_mass):
    """-> s [3] descending, q [4] canonical, density of the Gaussian with covariance cov and mass total_mass."""
    lam, vec = np.linalg.eigh(cov)
    lam, vec = lam[::-1], vec[:, ::-1]
    R = vec.T.copy()
    if np.linalg.det(R) < 0:
        R[2] = -R[2]
    s = np.sqrt(lam)
    return s, canonical_quat(R), total_mass / (s[0] * s[1] * s[2])


# ---- matching
def _directed(idx, cost, max_cost):
    idx = np.asarray(idx)
    cost = np.asarray(cost)
    P, K = idx.shape
    i = np.repeat(np.arange(P, dtype=np.int64), K)
    j = idx.reshape(-1).astype(np.int64)
    c = cost.reshape(-1)
    with np.errstate(invalid="ignore"):
        ok = (j >= 0) & (j < P) & (j != i) & (c <= max_cost)
    i, j, c = i[ok], j[ok], c[ok]
    return i, j, c, np.minimum(i, j), np.maximum(i, j)


def greedy_match(idx, cost, max_cost):
    """The sequential greedy matching: the eligible directed edges in (cost, min, max) order, an edge taken when both ends are
    free.  -> mate [P] int32."""
    P = np.asarray(idx).shape[0]
    i, j, c, lo, hi = _directed(idx, cost, max_cost)
    mate = np.full(P, -1, dtype=np.int32)
    for e in np.lexsort((hi, lo, c)):
        if mate[i[e]] < 0 and mate[j[e]] < 0:
            mate[i[e]], mate[j[e]] = j[e], i[e]
    return mate


def _point(P, i, j, c, lo, hi, mate):
    """ptr [P]: the partner of every unmatched node's smallest-key edge to an unmatched node, -1 where there is none."""
    free = mate < 0
    live = free[i] & free[j]
    node = np.concatenate([i[live], j[live]])
    other = np.concatenate([j[live], i[live]])
    cc, l2, h2 = (np.concatenate([t[live], t[live]]) for t in (c, lo, hi))
    order = np.lexsort((h2, l2, cc, node))
    node, other = node[order], other[order]
    first = np.ones(node.size, dtype=bool)
    first[1:] = node[1:] != node[:-1]
    ptr = np.full(P, -1, dtype=np.int64)
    ptr[node[first]] = other[first]
    return ptr


def round_match(idx, cost, max_cost, rounds=None):
    """The round-limited rule: per round every unmatched node points at the partner of its smallest-key eligible edge (own row and
    incoming edges), and nodes that point at each other are matched.  rounds = None: until nothing is left to point at.
    -> (mate [P] int32, rounds that matched something)."""
    P = np.asarray(idx).shape[0]
    i, j, c, lo, hi = _directed(idx, cost, max_cost)
    mate = np.full(P, -1, dtype=np.int32)
    done = 0
    while rounds is None or done < rounds:
        ptr = _point(P, i, j, c, lo, hi, mate)
        n = np.flatnonzero(ptr >= 0)
        if n.size == 0:
            break
        mutual = n[ptr[ptr[n]] == n]
        mate[mutual] = ptr[mutual]
        done += 1
    return mate, done


def open_count(idx, cost, max_cost, mate):
    P = np.asarray(idx).shape[0]
    i, j, c, lo, hi = _directed(idx, cost, max_cost)
    return int((_point(P, i, j, c, lo, hi, np.asarray(mate)) >= 0).sum())


def validate_mate(mate, density, scaling):
    """Entries out of range, self mates, one-sided entries and pairs with an end of non-positive or non-finite mass become -1."""
    mate = np.asarray(mate).astype(np.int64)
    P = mate.shape[0]
    m = mass(density, scaling)
    with np.errstate(invalid="ignore"):
        good = (m > 0) & np.isfinite(m)
    rng = (mate >= 0) & (mate < P)
    j = np.where(rng, mate, 0)
    ok = rng & (j != np.arange(P)) & (mate[j] == np.arange(P)) & good & good[j]
    return np.where(ok, mate, -1).astype(np.int32)


def merge_cloud(mate, xyz, density, scaling, rotation):
    """-> dict(src [Pn, 2] int32, xyz, density [Pn], scaling, rotation, cov [Pn, 3, 3], mass [Pn]) in float64: rows in ascending
    original index, a pair at its lower index.  Unmerged rows carry the inputs."""
    v = validate_mate(mate, density, scaling)
    P = v.shape[0]
    rows = np.flatnonzero(~((v >= 0) & (v < np.arange(P))))
    src = np.stack([rows, v[rows]], 1).astype(np.int32)
    x, d, s, q = (np.array(t, dtype=np.float64) for t in (xyz, density, scaling, rotation))
    d = d.reshape(-1)
    out = dict(src=src, xyz=x[rows].copy(), density=d[rows].copy(), scaling=s[rows].copy(), rotation=q[rows].copy())
    with np.errstate(all="ignore"):
        out["cov"] = covariance(s, q)[rows]
        out["mass"] = mass(d, s)[rows]
    mrows = np.flatnonzero(src[:, 1] >= 0)
    if mrows.size:
        _alpha, mu, cab, mt = pair_moments(src[mrows, 0], src[mrows, 1], x, d, s, q)
        for n, r in enumerate(mrows):
            sc, qq, rho = merged_row(cab[n], mt[n])
            out["xyz"][r], out["scaling"][r], out["rotation"][r], out["density"][r] = mu[n], sc, qq, rho
            out["cov"][r], out["mass"][r] = cab[n], mt[n]
    return out


# ---- clouds and graphs for the tests
def path_graph(n):
    """0 - 1 - 2 - ... with costs that grow along the path, both directions listed."""
    idx = np.full((n, 2), -1, dtype=np.int32)
    cost = np.full((n, 2), np.inf, dtype=np.float32)
    for i in range(n):
        if i + 1 < n:
            idx[i, 0], cost[i, 0] = i + 1, n - i    # the cheapest edge is the last: one pair per round from the far end
        if i > 0:
            idx[i, 1], cost[i, 1] = i - 1, n - i + 1
    return idx, cost


def random_cloud(P, seed, anisotropy=100.0, extent=1.0, scale=0.05):
    """P random Gaussians in float32: scales log-uniform within `anisotropy` of each other, random unit quaternions."""
    rng = np.random.RandomState(seed)
    xyz = rng.uniform(-extent, extent, (P, 3)).astype(np.float32)
    density = rng.uniform(0.1, 2.0, (P, 1)).astype(np.float32)
    scaling = (scale * np.exp(rng.uniform(-0.5, 0.5, (P, 3)) * np.log(anisotropy))).astype(np.float32)
    q = rng.normal(size=(P, 4))
    rotation = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)
    return xyz, density, scaling, rotation
