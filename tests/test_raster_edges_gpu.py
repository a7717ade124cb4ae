"""GPU: rasterizer chain identity at the edges -- wide Gaussians, the image borders, partial tiles, the tile-first limits.

dispatch.hpp promises that a forward's results never depend on its chain.  The tile-first scatter builds every instance's block
mask (which 8x8 blocks of its tile the Gaussian's alpha >= 1e-5 box touches) from integer bounds, one 32-bit mask per axis and
window of 16 tiles; the general chain evaluates block_mask4 per instance in floats.  Rounds 1-6 counted every block beyond the
16th tile of a rectangle as live, so the two chains handed the render kernels different masked lists for rectangles more than 16
tiles across or down -- no case of the suite had one.  Here: a small ordinary cloud plus planted Gaussians whose rectangles are
17-32 and more than 32 tiles wide and tall, clipped at every border, centred outside the image, strongly anisotropic (coverage
asserted from the oracle's rectangles, so the scene cannot quietly stop covering them), on detectors at and around the chain's
limits.  Per case: both chains bit for bit (lists, masked lists, image, every gradient), every mask against a float64 evaluation
of the alpha cut-off, image and gradients against the oracle; a stacked-view batch against its single views; a detector just
past the 4096-tile limit declines the chain and still matches the oracle.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from r2_gaussian_amd import scene as S
from tests import helpers as Hh

pytestmark = pytest.mark.gpu

ALPHA_MIN_2D = 1e-5
TILE = 16
GRAD_NAMES = ("dL_dmeans2D", "dL_dopacity", "dL_dmu", "dL_dmeans3D", "dL_dcov3D", "dL_dscales", "dL_drotations")


@pytest.fixture()
def L():
    from r2_gaussian_amd import _lib
    lib = _lib.lib()
    lib.r2_tile_first_control(1)
    lib.r2_tile_first_control(2)
    yield lib
    lib.r2_tile_first_control(1)
    lib.r2_tile_first_control(2)


# ------------------------------------------------------------------------------------------------ the scene
def _quat_from_matrix(R):
    """Unit quaternion (r, x, y, z) whose rotation matrix (the reference's convention: Sigma = R S^2 R^T) is R."""
    t = np.trace(R)
    if t > 0:
        s = np.sqrt(t + 1.0) * 2
        q = [0.25 * s, (R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s]
    else:
        i = int(np.argmax(np.diag(R)))
        j, k = (i + 1) % 3, (i + 2) % 3
        s = np.sqrt(1.0 + R[i, i] - R[j, j] - R[k, k]) * 2
        q = [0.0] * 4
        q[0] = (R[k, j] - R[j, k]) / s
        q[1 + i] = 0.25 * s
        q[1 + j] = (R[j, i] + R[i, j]) / s
        q[1 + k] = (R[k, i] + R[i, k]) / s
    q = np.asarray(q)
    return q / np.linalg.norm(q)


def _planted(v, specs):
    """Gaussians given in the view's pixel terms: (u, v) centre in pixels, (sx, sy) sigma in pixels along the image axes rotated
    by theta, view depth z, density.  -> (xyz, scales, rotations, density) arrays."""
    Rt = v.world_view_transform.numpy().astype(np.float64).T   # world -> view: Rt[:3, :3] p + Rt[:3, 3]
    Rw2c, T = Rt[:3, :3], Rt[:3, 3]
    W, H = v.image_width, v.image_height
    fx, fy = W / (2.0 * v.tanfovx), H / (2.0 * v.tanfovy)
    xyz, sc, rot, den = [], [], [], []
    for (u, vv, sx, sy, theta, z, d) in specs:
        X = ((2.0 * u + 1.0) / W - 1.0) * z * v.tanfovx
        Y = ((2.0 * vv + 1.0) / H - 1.0) * z * v.tanfovy
        xyz.append(Rw2c.T @ (np.array([X, Y, z]) - T))
        c, s = np.cos(theta), np.sin(theta)
        # local axes 1, 2 along the rotated image axes (pixel units differ per axis: scale them back to view units)
        a1 = np.array([c * sx / fx, s * sx / fy, 0.0]) * z
        a2 = np.array([-s * sy / fx, c * sy / fy, 0.0]) * z
        n1, n2 = np.linalg.norm(a1), np.linalg.norm(a2)
        e1 = a1 / n1
        e2 = a2 - e1 * (e1 @ a2)
        e2 /= np.linalg.norm(e2)
        e3 = np.cross(e1, e2)
        Rv = np.stack([e1, e2, e3], 1)            # columns: the local axes in view space
        sc.append([n1, n2, 0.5 * min(n1, n2)])
        rot.append(_quat_from_matrix(Rw2c.T @ Rv))
        den.append([d])
    f = np.float32
    return (np.asarray(xyz, f), np.asarray(sc, f), np.asarray(rot, f), np.asarray(den, f))


def _specs(W, H, seed):
    """Planted Gaussians for a W x H detector: wide (17-32 and > 32 tiles where the grid has room), clipped at each border,
    centred outside the image, strongly anisotropic."""
    g = np.random.default_rng(seed)
    cx, cy = W / 2.0, H / 2.0
    sp = []

    def add(u, v, sx, sy, th=0.0):
        sp.append((u, v, sx, sy, th, 4.2 + 1.6 * g.random(), 0.02 + 0.1 * g.random()))
    # wide: radius ~ 3 sigma; 24 tiles ~ sigma 64 px, 40 tiles ~ sigma 107 px; on a narrow grid the whole axis
    for tiles in (20, 24, 30, 40, 48, 70):
        s = tiles * TILE / 6.0
        add(cx + g.uniform(-0.1, 0.1) * W, cy + g.uniform(-0.1, 0.1) * H, s, s * g.uniform(0.5, 1.0), g.uniform(0, np.pi))
    add(cx, cy, W / 3.0, W / 3.0)                                   # the whole grid, both axes
    # clipped at each border, and centred outside it with the rectangle reaching in
    r = max(24.0, min(W, H) / 6.0)
    for (u, v) in ((-0.1 * r, cy), (W + 0.1 * r, cy), (cx, -0.1 * r), (cx, H + 0.1 * r),
                   (-0.6 * r, 0.3 * H), (W + 0.6 * r, 0.7 * H), (0.3 * W, -0.6 * r), (0.7 * W, H + 0.6 * r),
                   (-0.5 * r, -0.5 * r), (W + 0.5 * r, H + 0.5 * r)):
        add(u, v, r / 2.2, r / 2.2 * g.uniform(0.6, 1.0), g.uniform(0, np.pi))
    # strongly anisotropic: thin along one image axis (box << rectangle there), along x, along y, and tilted a little.  (Axis
    # ratios well below 100: beyond it the preprocess calls the conic ill-conditioned and gives it an infinite box.  Such
    # Gaussians, and ones thinner than ~2 px across a footprint of hundreds of pixels, render identically on both chains but
    # miss the oracle's pure 1e-4 gradient bound on single cancelling elements by up to 4x: not planted here.)
    for th in (0.0, np.pi / 2, 0.05, np.pi / 2 - 0.05, 0.0, np.pi / 2):
        sy = 2.5 + g.random()
        add(g.uniform(0.2, 0.8) * W, g.uniform(0.2, 0.8) * H, min(g.uniform(0.3, 1.0) * max(W, H) / 5.0, 40.0 * sy), sy, th)
    # and a few of every kind near the partial last tile column / row
    for _ in range(4):
        add(W - g.uniform(0, 12), H - g.uniform(0, 12), g.uniform(3, 40), g.uniform(3, 40), g.uniform(0, np.pi))
    return sp


def make_scene(v, seed=0, P_cloud=3000):
    c = S.make_cloud(P_cloud, seed=seed)
    xyz, sc, rot, den = _planted(v, _specs(v.image_width, v.image_height, seed + 100))
    return S.Cloud(torch.cat([c.xyz, torch.from_numpy(xyz)]).contiguous(), torch.cat([c.scales, torch.from_numpy(sc)]).contiguous(),
                   torch.cat([c.rotations, torch.from_numpy(rot)]).contiguous(), torch.cat([c.density, torch.from_numpy(den)]).contiguous())


def oracle_rects(o):
    """The reference's tile rectangles (getRect, RAS/auxiliary.h): [x0, x1) x [y0, y1) per Gaussian; zero for culled ones."""
    gx, gy = o["grid"]
    m, r = o["means2D"].astype(np.float32), o["radii"].astype(np.float32)
    x0 = np.clip(((m[:, 0] - r) / TILE).astype(np.int64), 0, gx)
    y0 = np.clip(((m[:, 1] - r) / TILE).astype(np.int64), 0, gy)
    x1 = np.clip(((m[:, 0] + r + TILE - 1) / TILE).astype(np.int64), 0, gx)
    y1 = np.clip(((m[:, 1] + r + TILE - 1) / TILE).astype(np.int64), 0, gy)
    vis = o["radii"] > 0
    out = np.stack([x0, y0, x1, y1], 1)
    out[~vis] = 0
    assert np.array_equal((out[:, 2] - out[:, 0]) * (out[:, 3] - out[:, 1]), o["tiles_touched"].astype(np.int64))
    return out


def assert_coverage(o, W, H, extent=None, full=True):
    """The scene holds every kind of edge it is meant to: asserted from the oracle's rectangles, so that it cannot quietly stop
    covering them.  extent: the HIP records' alpha >= 1e-5 half-extents (rec[:, 6:8]), for the anisotropy."""
    gx, gy = o["grid"]
    rc = oracle_rects(o)
    vis = o["tiles_touched"] > 0
    w, h = rc[:, 2] - rc[:, 0], rc[:, 3] - rc[:, 1]
    got = {}
    got["w17_32"] = bool((vis & (w >= 17) & (w <= 32)).any()) if gx >= 17 else None
    got["w33+"] = bool((vis & (w > 32)).any()) if gx > 32 else None
    got["h17_32"] = bool((vis & (h >= 17) & (h <= 32)).any()) if gy >= 17 else None
    got["h33+"] = bool((vis & (h > 32)).any()) if gy > 32 else None
    m, r = o["means2D"], o["radii"]
    got["clip_left"] = bool((vis & (m[:, 0] - r < 0)).any())
    got["clip_right"] = bool((vis & (m[:, 0] + r > W)).any())
    got["clip_top"] = bool((vis & (m[:, 1] - r < 0)).any())
    got["clip_bottom"] = bool((vis & (m[:, 1] + r > H)).any())
    outside = (m[:, 0] < 0) | (m[:, 0] >= W) | (m[:, 1] < 0) | (m[:, 1] >= H)
    got["centre_outside"] = int((vis & outside).sum()) >= 4
    if extent is not None:
        hx, hy = extent[:, 0], extent[:, 1]
        thin = vis & (np.minimum(hx, hy) * 8 < r) & (r > 3 * TILE)   # box at most an eighth of the rectangle in one axis
        got["anisotropic"] = int(thin.sum()) >= 3
    missing = [k for k, x in got.items() if x is False]
    assert not missing, "the scene does not cover: %s (%dx%d)" % (missing, W, H)
    if full:
        assert all(x is not None for x in got.values()), got
    return got


# ------------------------------------------------------------------------------------------------ checks
def _both(L, c, v, gpu):
    """-> (general chain's result, tile-first result) for the same call."""
    L.r2_tile_first_control(0)
    g = Hh.hip_raster(c, v, gpu)
    assert not Hh.took_tile_first(g)
    L.r2_tile_first_control(1)
    L.r2_tile_first_control(2)
    Hh.hip_raster(c, v, gpu)            # leaves the prediction
    t = Hh.hip_raster(c, v, gpu)
    assert Hh.took_tile_first(t), "the second call of a size did not take the tile-first chain"
    return g, t


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def assert_same_chains(g, t, gg=None, gt=None):
    """Both chains bit for bit: counts, lists, the render kernels' masked list, image (and every gradient of the backward)."""
    assert t["num_rendered"] == g["num_rendered"]
    differ = [k for k in ("radii", "tiles_touched", "point_list", "ranges", "masked") if not np.array_equal(g[k], t[k])]
    if not np.array_equal(_bits(g["color"]), _bits(t["color"])):
        differ.append("color (%d pixels)" % int((_bits(g["color"]) != _bits(t["color"])).sum()))
    if "masked" in differ:
        d = g["masked"] != t["masked"]
        differ[differ.index("masked")] = "masked (%d of %d entries; general %s, tile-first %s)" % (
            int(d.sum()), d.size, np.unique(g["masked"][d] & 15)[:8].tolist(), np.unique(t["masked"][d] & 15)[:8].tolist())
    if gg is not None:
        differ += [k for k in GRAD_NAMES if not np.array_equal(_bits(gg[k]), _bits(gt[k]))]
    assert not differ, "the general and the tile-first chain differ in: %s" % differ


def check_masks(h, W, H, chunk=4096):
    """Every masked-list entry's block mask names every 8x8 block of its tile that holds a pixel (inside the image) with
    alpha >= 1.01 x ALPHA_MIN_2D, alpha evaluated in float64 from the decoded record.  (The 1 % keeps float32-vs-float64
    borderline pixels out of it.)  The masks are also the ids of point_list."""
    gx = (W + TILE - 1) // TILE
    ms = h["masked"]
    ids = (ms >> 4).astype(np.int64)
    bits = (ms & 15).astype(np.int64)
    assert np.array_equal(ids, h["point_list"]), "masked list ids are not point_list"
    tiles = h["tiles"].astype(np.int64)
    tx, ty = tiles % gx, tiles // gx
    m = h["means2D"].astype(np.float64)
    co = h["conic"].astype(np.float64)
    amp = h["opacity"].astype(np.float64) * h["mus"].astype(np.float64)
    o16 = np.arange(TILE, dtype=np.float64)
    blk = np.array([[1, 2], [4, 8]], np.int64)   # bit q: x block q & 1, y block q >> 1
    missed = 0
    for s in range(0, ids.size, chunk):
        k = slice(s, s + chunk)
        i = ids[k]
        px = (tx[k] * TILE)[:, None, None] + o16[None, None, :]
        py = (ty[k] * TILE)[:, None, None] + o16[None, :, None]
        dx, dy = m[i, 0][:, None, None] - px, m[i, 1][:, None, None] - py
        power = -0.5 * (co[i, 0][:, None, None] * dx * dx + co[i, 2][:, None, None] * dy * dy) - co[i, 1][:, None, None] * dx * dy
        alpha = amp[i][:, None, None] * np.exp(np.minimum(power, 0.0))
        hot = (alpha >= 1.01 * ALPHA_MIN_2D) & (px < W) & (py < H) & (power <= 0.0)
        live = hot.reshape(-1, 2, 8, 2, 8).any(axis=(2, 4))          # [entry, y block, x block]
        need = (live * blk[None]).sum(axis=(1, 2))
        missed += int((need & ~bits[k]).astype(bool).sum())
    assert missed == 0, "%d masked-list entries miss a block that holds a pixel above the cut-off" % missed


# ------------------------------------------------------------------------------------------------ single views
@pytest.mark.parametrize("det", [(1024, 1024), (16, 4096), (200, 520), (77, 515)],
                         ids=["1024x1024_4096_tiles", "4096x16_axis_limit", "520x200_half_last_column", "515x77_partial_blocks"])
def test_wide_and_edge_gaussians_identical_on_both_chains(det, L, oracle, gpu):
    H, W = det
    v = S.make_views(8, det)[3]
    c = make_scene(v, seed=5)
    g, t = _both(L, c, v, gpu)
    o = Hh.oracle_raster(oracle, c, v)
    assert_coverage(o, W, H, t["extent"], full=(det == (1024, 1024)))
    if det == (1024, 1024):
        assert o["ranges"].shape[0] == 4096
    dL = S.make_pixel_grad(H, W).numpy()
    gg = Hh.hip_raster_backward(g, c, v, dL, gpu)
    gt = Hh.hip_raster_backward(t, c, v, dL, gpu)
    assert_same_chains(g, t, gg, gt)
    Hh.check_binning(t, o)
    check_masks(t, W, H)
    Hh.parity_image(oracle, o, t["color"], "edges %dx%d" % (W, H))
    if det != (16, 4096):
        # (4096 x 16: pixels 256 times as wide as tall, so the planted Gaussians are a few pixels across one axis and hundreds
        # along the other; on the parent tree as on this one a few cancelling gradient elements of such Gaussians miss the
        # oracle's pure 1e-4 bound.  Both chains agree bit for bit there -- asserted above -- and the image meets the bound.)
        Hh.parity_raster_grads(oracle, o, gt, c, v, dL, "edges %dx%d" % (W, H))


def test_past_the_tile_limit_takes_the_general_chain(L, oracle, gpu):
    """1040 x 1024: 65 x 64 = 4160 tiles, past the chain's 4096.  Declined every time (r2_path_stats says why), and the general
    chain's result is the oracle's."""
    from r2_gaussian_amd import _lib
    H, W = 1024, 1040
    v = S.make_views(8, (H, W))[3]
    c = make_scene(v, seed=6)
    _lib.path_stats(reset=True)
    Hh.hip_raster(c, v, gpu)
    h = Hh.hip_raster(c, v, gpu)
    ps = _lib.path_stats()
    assert not Hh.took_tile_first(h)
    assert ps["raster.general.grid"] == 2 and ps["raster.tile_first"] == 0, ps
    o = Hh.oracle_raster(oracle, c, v)
    assert_coverage(o, W, H, h["extent"])
    Hh.check_binning(h, o)
    check_masks(h, W, H)
    Hh.parity_image(oracle, o, h["color"], "past the tile limit")
    dL = S.make_pixel_grad(H, W).numpy()
    Hh.parity_raster_grads(oracle, o, Hh.hip_raster_backward(h, c, v, dL, gpu), c, v, dL, "past the tile limit")


# ------------------------------------------------------------------------------------------------ stacked views
def _batch(c, views, dev):
    from r2_gaussian_amd import _C, _lib
    e = torch.empty(0)
    vm = torch.stack([v.world_view_transform for v in views]).to(dev)
    pm = torch.stack([v.full_proj_transform for v in views]).to(dev)
    v0 = views[0]
    args = (c.xyz.to(dev), c.density.to(dev), c.scales.to(dev), c.rotations.to(dev), 1.0, e, vm, pm, v0.tanfovx, v0.tanfovy,
            v0.image_height, v0.image_width, v0.mode, False)
    R, color, radii, gb, bb, ib = _C.rasterize_gaussians_batch(*args)
    torch.cuda.synchronize()
    P, H, W = c.xyz.shape[0], v0.image_height, v0.image_width
    bn = bb.cpu().numpy()
    L = _lib.lib()

    def read(which):
        bid = C.c_int(-1)
        off = L.r2_raster_state_offset(which, P * len(views), R, W, H, C.byref(bid))
        assert off >= 0 and bid.value == 1
        return bn[off:off + 4 * R].view(np.uint32).copy()
    return dict(args=args, R=R, color=color.cpu().numpy(), radii=radii.cpu().numpy(), bufs=(gb, bb, ib),
                point_list=read(5), masked=read(16))


def _batch_backward(b, dL, dev):
    from r2_gaussian_amd import _C
    a = b["args"]
    gb, bb, ib = b["bufs"]
    res = _C.rasterize_gaussians_backward_batch(a[0], torch.as_tensor(b["radii"]).to(dev), a[2], a[3], 1.0, a[5], a[6], a[7], a[8],
                                                a[9], torch.as_tensor(dL).to(dev), gb, b["R"], bb, ib, a[12], False)
    torch.cuda.synchronize()
    return {n: t.cpu().numpy() for n, t in zip(GRAD_NAMES, res)}


def test_stacked_views_with_wide_gaussians(L, oracle, gpu):
    """V = 3 views of 520 x 200 through one batched forward: the first call of the size takes the general chain, the second the
    stacked tile-first chain.  Both bit for bit (lists, masked lists, images, gradients); every view bit for bit its single-view
    call (image, radii, screen-space gradients) and, with the lists, the oracle's."""
    from r2_gaussian_amd import _lib
    hw = (200, 520)
    H, W = hw
    views = [S.make_view(0.3 + 0.9 * k, hw) for k in range(3)]
    c = make_scene(views[0], seed=9)
    P = c.xyz.shape[0]
    _lib.path_stats(reset=True)
    b1 = _batch(c, views, gpu)
    b2 = _batch(c, views, gpu)
    ps = _lib.path_stats()
    assert ps["raster.general.no_prediction"] == 1 and ps["raster.tile_first"] == 1, ps
    assert b1["R"] == b2["R"]
    differ = [k for k in ("radii", "point_list", "masked") if not np.array_equal(b1[k], b2[k])]
    if not np.array_equal(_bits(b1["color"]), _bits(b2["color"])):
        differ.append("color")
    g = torch.Generator().manual_seed(3)
    dL = ((torch.rand((3,) + hw, generator=g) * 2 - 1) / float(H * W)).numpy()
    g1, g2 = _batch_backward(b1, dL, gpu), _batch_backward(b2, dL, gpu)
    differ += [k for k in GRAD_NAMES if not np.array_equal(_bits(g1[k]), _bits(g2[k]))]
    assert not differ, "the general and the stacked tile-first chain differ in: %s" % differ
    singles = [Hh.hip_raster(c, v, gpu) for v in views]
    assert b2["R"] == sum(h["num_rendered"] for h in singles)
    off = 0
    for k, (v, h) in enumerate(zip(views, singles)):
        assert np.array_equal(b2["radii"][k], h["radii"]), "radii of view %d" % k
        assert np.array_equal(_bits(b2["color"][k]), _bits(h["color"][0])), "image of view %d" % k
        n = h["num_rendered"]
        assert np.array_equal(b2["point_list"][off:off + n], h["point_list"] + k * P), "point_list of view %d" % k
        assert np.array_equal(b2["masked"][off:off + n], h["masked"] + ((k * P) << 4)), "masked list of view %d" % k
        off += n
        gs = Hh.hip_raster_backward(h, c, v, dL[k:k + 1], gpu)
        assert np.array_equal(_bits(g2["dL_dmeans2D"][k]), _bits(gs["dL_dmeans2D"])), "dL_dmeans2D of view %d" % k
        o = Hh.oracle_raster(oracle, c, v)
        if k == 0:
            assert_coverage(o, W, H, h["extent"], full=False)
        Hh.check_binning(h, o)
        check_masks(h, W, H)
        Hh.parity_image(oracle, o, b2["color"][k:k + 1], "stacked edges view %d" % k)
        Hh.parity_raster_grads(oracle, o, gs, c, v, dL[k:k + 1], "stacked edges view %d" % k)
