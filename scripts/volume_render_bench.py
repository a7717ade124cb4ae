"""Timing of the direct volume renderer (csrc/volume_render.hip) on the MI355X; prints one JSON line.

    python scripts/volume_render_bench.py [--n 256] [--size 1000 800] [--rounds 5] [--reps 50] [--torch_rounds 2] [--once]

Workload: plot_volume.py's picture at the driver's defaults -- a window 800 wide and 1000 high, the script's camera, viridis,
the "linear" opacity ramp over clim [0, 1], accuracy 0.5, the leading half of the volume along x zeroed -- of two seeded 256^3
phantoms: "smooth", recon_bench.py's two Gaussian blobs, which are nowhere exactly zero (so only the cut half is empty), and
"ct", constant ellipsoids in exact-zero air, which is what a CT volume seen through a ramp looks like.

Entries, each through volume_render.py: render (brick table reused, t_stop 2^-10: the default), render_nobricks, render_nostop
(table, t_stop 0), render_plain (neither), mip, mip_nobricks and bricks (r2_volume_bricks alone).  Yardsticks in the same run:
project (projector.project_rays on the same rays and accuracy: the same gathers with no classification -- the floor this
kernel can be priced against) and torch (the same renderer composed of library calls: grid_sample per slab of samples and
cumulative products; the rendering a user would otherwise write).  --reps calls between two device events after one warm-up
call each; the median and minimum over --rounds windows, the rounds alternating between the entries.  Other people's work
shares the machine: compare numbers of one run only.

Per entry: ms; samples / s over the samples of the full walk (sum of n over the rays that hit).  Per phantom: the fraction of
those samples that lie in bricks the compositing kernel tests empty (counted by the torch composition's walk from the kernel's
own brick table), the fraction of rays that stop early (final transmittance below t_stop), and the largest difference between
the torch composition and the kernel (they round differently; it is reported, not asserted).

--once runs every kernel entry a single time and nothing else: the command to put under a counter collection.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from r2_gaussian_amd import projector as PJ          # noqa: E402
from r2_gaussian_amd import volume_render as VR      # noqa: E402

T_STOP = 2.0 ** -10
SLAB = 16


def event_ms(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def phantoms(n, dev):
    ax = torch.linspace(-1 + 1.0 / n, 1 - 1.0 / n, n, device=dev)
    X, Y, Z = torch.meshgrid(ax, ax, ax, indexing="ij")
    smooth = (0.6 * torch.exp(-((X - 0.1) ** 2 + (Y + 0.2) ** 2 + Z ** 2) / 0.18)
              + 0.5 * torch.exp(-((X + 0.3) ** 2 + (Y - 0.25) ** 2 + (Z + 0.1) ** 2) / 0.03))
    ct = torch.zeros_like(smooth)

    def ellipsoid(c, r, value):
        inside = ((X - c[0]) / r[0]) ** 2 + ((Y - c[1]) / r[1]) ** 2 + ((Z - c[2]) / r[2]) ** 2 <= 1
        ct[inside] = value

    ellipsoid((0, 0, 0), (0.8, 0.6, 0.85), 0.25)          # the body
    ellipsoid((0.3, 0.0, 0.0), (0.28, 0.35, 0.5), 0.05)   # two lungs
    ellipsoid((-0.3, 0.0, 0.0), (0.28, 0.35, 0.5), 0.05)
    ellipsoid((0.0, 0.42, 0.0), (0.08, 0.08, 0.8), 0.9)   # a spine
    ellipsoid((0.0, -0.1, 0.1), (0.12, 0.15, 0.15), 0.5)  # a heart
    out = {}
    for name, v in (("smooth", smooth), ("ct", ct)):
        v = v.contiguous()
        v[: n // 2] = 0                                     # plot_volume.py: half set to zero to show the inner structure
        out[name] = v
    return out


def torch_render(vol, rays, H, W, dVoxel, accuracy, lut, clim, empty=None):
    """One perspective view composed of torch calls -> ([H,W,4], samples, samples in empty bricks).  The walk follows the
    contract (clip to [-1, n], n = ceil(L / accuracy) midpoint samples); its roundings are torch's, not the kernel's."""
    dev = vol.device
    R = torch.as_tensor(rays[0], device=dev)
    n3 = torch.tensor(vol.shape, device=dev, dtype=torch.float32)
    c, r = torch.meshgrid(torch.arange(W, device=dev, dtype=torch.float32), torch.arange(H, device=dev, dtype=torch.float32), indexing="xy")
    s = R[0:3]
    d = (R[3:6] + c.reshape(-1, 1) * R[6:9] + r.reshape(-1, 1) * R[9:12]) - s
    ta, tb = (-1.0 - s) / d, (n3 - s) / d
    t0 = torch.minimum(ta, tb).amax(1).clamp_min(0.0)
    t1 = torch.maximum(ta, tb).amin(1)
    hit = t1 > t0
    span = torch.where(hit, t1 - t0, torch.zeros_like(t0))
    n = torch.where(hit, torch.ceil(span * d.norm(dim=1) / accuracy).clamp_min(1.0), torch.zeros_like(t0))
    dt = span / n.clamp_min(1.0)
    dl = dt * (d * torch.tensor(dVoxel, device=dev)).norm(dim=1)
    K = lut.shape[0]
    scale = (K - 1) / (clim[1] - clim[0])
    C = torch.zeros((H * W, 3), device=dev)
    T = torch.ones(H * W, device=dev)
    v5 = vol[None, None]
    in_empty = 0
    for k0 in range(0, int(n.max().item()), SLAB):
        k = torch.arange(k0, k0 + SLAB, device=dev, dtype=torch.float32)
        t = t0[:, None] + (k + 0.5) * dt[:, None]
        q = s + t[..., None] * d[:, None, :]                                   # [R, SLAB, 3]
        g = (2.0 * q / (n3 - 1).clamp_min(1.0) - 1.0).flip(-1)                 # grid_sample wants (z, y, x) order reversed
        f = torch.nn.functional.grid_sample(v5, g[None, :, :, None, :], mode="bilinear", padding_mode="zeros", align_corners=True)[0, 0, :, :, 0]
        live = k < n[:, None]
        x = ((f - clim[0]) * scale).clamp(0.0, K - 1.0)
        i = x.floor().clamp_max(K - 2.0).long()
        w = (x - i)[..., None]
        ch = lut[i] + w * (lut[i + 1] - lut[i])
        e = torch.where(live, torch.exp(-ch[..., 3] * dl[:, None]), torch.ones_like(f))
        Tk = T[:, None] * torch.cumprod(torch.cat([torch.ones_like(e[:, :1]), e[:, :-1]], 1), 1)   # transmittance before sample k
        C = C + ((Tk * (1 - e))[..., None] * ch[..., :3]).sum(1)
        T = Tk[:, -1] * e[:, -1]
        if empty is not None:
            b = (q.floor().long().clamp_min(0).minimum((n3 - 1).long()) >> 3)
            nb = empty.shape
            in_empty += int((empty.reshape(-1)[(b[..., 0] * nb[1] + b[..., 1]) * nb[2] + b[..., 2]] & live).sum().item())
    return torch.cat([C, (1 - T)[:, None]], 1).reshape(H, W, 4), int(n.sum().item()), in_empty


def empty_table(table, lut, clim):
    """The compositing kernel's test on its brick table, in torch (include/r2hip.h: r2_render_volume)."""
    K = lut.shape[0]
    mn, mx = table[..., 0], table[..., 1]
    pad = torch.maximum(mn.abs(), mx.abs()) * 2.0 ** -21
    lo, hi = mn - pad, mx + pad
    lo, hi = torch.nextafter(lo, lo - pad), torch.nextafter(hi, hi + pad)
    scale = torch.tensor(K - 1, dtype=torch.float32) / (torch.tensor(clim[1], dtype=torch.float32) - torch.tensor(clim[0], dtype=torch.float32))
    xa = ((lo - clim[0]) * scale.to(lo.device)).clamp(0.0, K - 1.0)
    xb = ((hi - clim[0]) * scale.to(lo.device)).clamp(0.0, K - 1.0)
    ia, ib = xa.floor().clamp_max(K - 2.0).long(), xb.floor().clamp_max(K - 2.0).long()
    last = torch.where(xb > ib, ib + 1, ib)
    nzp = torch.cat([torch.zeros(1, dtype=torch.long, device=lut.device), torch.cumsum((lut[:, 3] != 0).long(), 0)])
    return nzp[last + 1] == nzp[ia]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--size", type=int, nargs=2, default=[1000, 800], metavar=("H", "W"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--torch_rounds", type=int, default=2)
    ap.add_argument("--once", action="store_true", help="run every kernel entry once and nothing else (for a counter collection)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("volume_render_bench needs the GPU: a timing taken anywhere else says nothing")
    dev = torch.device("cuda:0")
    n, (H, W) = a.n, a.size
    sVoxel, center, clim, accuracy = [2.0, 2.0, 2.0], [0.0, 0.0, 0.0], (0.0, 1.0), 0.5
    dVoxel = [s / n for s in sVoxel]
    rays_h = VR.orbit_rays([VR.AZIMUTH], VR.ELEVATION, VR.DISTANCE * max(sVoxel), H, W, sVoxel, center, (n, n, n), fov_y=VR.FOV)
    rays = PJ.device_rays(rays_h, dev)
    lut = torch.from_numpy(VR.transfer_function("viridis", "linear", VR.default_unit(sVoxel, (n, n, n)))).to(dev)
    res = {"n": n, "H": H, "W": W, "rounds": a.rounds, "reps": a.reps, "accuracy": accuracy, "t_stop": T_STOP, "phantoms": {}}
    for name, vol in phantoms(n, dev).items():
        table = VR.volume_bricks(vol)
        out4 = torch.empty((1, H, W, 4), device=dev)
        out1 = torch.empty((1, H, W), device=dev)
        entries = {
            "render": lambda: VR.render_volume(vol, rays, True, H, W, dVoxel, lut, clim, accuracy, T_STOP, table, out4),
            "render_nobricks": lambda: VR.render_volume(vol, rays, True, H, W, dVoxel, lut, clim, accuracy, T_STOP, False, out4),
            "render_nostop": lambda: VR.render_volume(vol, rays, True, H, W, dVoxel, lut, clim, accuracy, 0.0, table, out4),
            "render_plain": lambda: VR.render_volume(vol, rays, True, H, W, dVoxel, lut, clim, accuracy, 0.0, False, out4),
            "mip": lambda: VR.mip(vol, rays, True, H, W, dVoxel, accuracy, table, out1),
            "mip_nobricks": lambda: VR.mip(vol, rays, True, H, W, dVoxel, accuracy, False, out1),
            "bricks": lambda: VR.volume_bricks(vol),
            "project": lambda: PJ.project_rays(vol, rays, True, H, W, dVoxel, accuracy, out1),
        }
        for fn in entries.values():
            fn()
        torch.cuda.synchronize()
        if a.once:
            continue
        ts = {k: [] for k in entries}
        for _ in range(a.rounds):
            for k, fn in entries.items():
                ts[k].append(event_ms(fn, a.reps))
        empty = empty_table(table, lut, clim)
        ref, samples, in_empty = torch_render(vol, rays_h, H, W, dVoxel, accuracy, lut, clim, empty)
        torch.cuda.synchronize()
        tt = [event_ms(lambda: torch_render(vol, rays_h, H, W, dVoxel, accuracy, lut, clim), 1) for _ in range(a.torch_rounds)]
        entries["render"]()
        stopped = float(((1 - out4[..., 3]) < T_STOP).float().mean().item())
        entries["render_plain"]()
        r = {"samples": samples, "empty_bricks": float(empty.float().mean().item()), "samples_in_empty_bricks": in_empty / max(samples, 1),
             "rays_with_opacity": float((out4[..., 3] > 0).float().mean().item()), "rays_stopped_early": stopped,
             "max_abs_torch_minus_kernel": float((ref - out4[0]).abs().max().item())}
        for k in entries:
            ms = float(np.median(ts[k]))
            r[k] = {"ms": ms, "ms_min": float(np.min(ts[k]))}
            if k != "bricks":
                r[k]["samples_per_s"] = samples / (ms * 1e-3)
        ms = float(np.median(tt))
        r["torch"] = {"ms": ms, "ms_min": float(np.min(tt)), "samples_per_s": samples / (ms * 1e-3), "ratio_to_render": ms / r["render"]["ms"]}
        res["phantoms"][name] = r
    print(json.dumps(res))


if __name__ == "__main__":
    main()
