"""Timing of the isosurface kernels (csrc/isosurface.hip) and of mesh.isosurface / mesh.snap_to_field on the MI355X; prints a
table and one JSON line.

    python scripts/mesh_bench.py [--sizes 128 256 512] [--rounds 9] [--reps 20]

Inputs, at n^3 for every n of --sizes: a sphere (0.7 - |x| on [-1, 1]^3, level 0: one smooth closed surface, O(n^2) triangles)
and a datagen-style volume (three Gaussian blobs plus seeded uniform noise of amplitude 0.02, level 0.3: a rough surface with
many small components, what a reconstruction looks like).

Timing.  r2_isosurface_count and r2_isosurface_fill are called through the C ABI, --reps calls back to back between two device
events (so a window is milliseconds, not a launch), after a warm-up at the size; the median and the minimum over --rounds
windows are reported, the rounds alternating between count and fill.  ``isosurface`` is the whole Python call -- workspace and
output allocation, both entries and the one host read of the counts between them -- on a host clock around a call that ends
in a device synchronise.  ``snap`` is one Newton iteration of mesh.snap_to_field on the mesh's vertices against a seeded
50 000-Gaussian cloud (scene.make_cloud): the difference of the medians of calls with 2 and with 1 iterations.

Bytes.  The algorithmic bytes are one read of the volume per pass that needs it, plus the workspace, plus the outputs:
  count  4 N (the volume, once: the seven neighbours of a point come from cache) + 2 N (mask and triangle count, written)
         + N (the mask, read by the base pass) + 4 Nv' (the first vertex id of every owner with a crossed edge, Nv' <= Nv);
         reported with Nv' = Nv
  fill   2 N (mask and triangle count, read) + 24 Nv (vertices and normals) + 12 Nt (faces) + per vertex two values of the
         volume and its id (12 Nv) + per triangle-bearing cell its eight values and seven owners' mask and id (counted as
         67 bytes per cell, cells <= Nt)
gbps = these bytes over the median time.  A 256^3 volume (64 MiB) sits in the 256 MiB Infinity Cache between calls: only the
512^3 row says something about HBM.  Other people's work shares the machine: compare numbers of one run only.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from r2_gaussian_amd import _lib                     # noqa: E402
from r2_gaussian_amd import mesh as MS               # noqa: E402
from r2_gaussian_amd import scene as S               # noqa: E402
from r2_gaussian_amd._boundary import call, workspace   # noqa: E402


def event_ms(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def sphere(n, dev):
    ax = torch.linspace(-1.0, 1.0, n, device=dev)
    X, Y, Z = torch.meshgrid(ax, ax, ax, indexing="ij")
    return (0.7 - torch.sqrt(X * X + Y * Y + Z * Z)).contiguous(), 0.0


def phantom(n, dev):
    ax = -1 + (torch.arange(n, device=dev, dtype=torch.float32) + 0.5) * (2.0 / n)
    X, Y, Z = torch.meshgrid(ax, ax, ax, indexing="ij")
    vol = torch.zeros((n, n, n), device=dev)
    for c0, sigma, rho in (((0.1, -0.2, 0.05), 0.3, 0.6), ((-0.3, 0.25, -0.1), 0.12, 0.5), ((0.35, 0.3, 0.2), 0.08, 0.4)):
        vol += rho * torch.exp(-((X - c0[0]) ** 2 + (Y - c0[1]) ** 2 + (Z - c0[2]) ** 2) / (2 * sigma ** 2))
    g = torch.Generator(device=dev).manual_seed(n)
    return (vol + 0.02 * torch.rand((n, n, n), device=dev, generator=g)).contiguous(), 0.3


def bench_volume(name, vol, level, rounds, reps, dev, cloud):
    n = vol.shape[0]
    N = vol.numel()
    ws = workspace(_lib.lib().r2_isosurface_workspace_bytes(n, n, n), dev, at_least=1)
    counts = torch.empty((3,), dtype=torch.int64, device=dev)

    def count():
        call("r2_isosurface_count", dev, n, n, n, vol, level, ws, ws.numel(), counts)

    count()
    nv, nt, bad = (int(c) for c in counts.cpu())
    assert bad == 0
    verts = torch.empty((nv, 3), device=dev)
    nrm = torch.empty((nv, 3), device=dev)
    faces = torch.empty((nt, 3), dtype=torch.int32, device=dev)

    def fill():
        call("r2_isosurface_fill", dev, n, n, n, vol, level, -1.0, -1.0, -1.0, 2.0 / n, 2.0 / n, 2.0 / n, ws, ws.numel(), nv, nt,
             verts, nrm, faces)

    def whole():
        MS.isosurface(vol, level, (0.0, 0.0, 0.0), (2.0, 2.0, 2.0))
        torch.cuda.synchronize()

    for fn in (count, fill, whole):
        fn()
    torch.cuda.synchronize()
    t = {"count": [], "fill": [], "isosurface": []}
    for _ in range(rounds):
        t["count"].append(event_ms(count, reps))
        t["fill"].append(event_ms(fill, reps))
        t0 = time.perf_counter()
        whole()
        t["isosurface"].append((time.perf_counter() - t0) * 1e3)
    nbytes = {"count": 7 * N + 4 * nv, "fill": 2 * N + 36 * nv + 12 * nt + 67 * nt}
    res = {"volume": name, "n": n, "verts": nv, "tris": nt, "workspace_bytes": int(ws.numel())}
    for k in t:
        res[k + "_ms"] = float(np.median(t[k]))
        res[k + "_ms_min"] = float(np.min(t[k]))
    for k in nbytes:
        res[k + "_bytes"] = nbytes[k]
        res[k + "_gbps"] = nbytes[k] / (res[k + "_ms"] * 1e-3) / 1e9
    # one Newton iteration of the snap, on this mesh's vertices
    v, _f, _n = MS.isosurface(vol, level, (0.0, 0.0, 0.0), (2.0, 2.0, 2.0), normals=False)
    if v.shape[0]:
        snap = {k: [] for k in (1, 2)}
        MS.snap_to_field(v, 0.3, *cloud, n_iter=1)
        torch.cuda.synchronize()
        for _ in range(max(3, rounds // 3)):
            for k in (1, 2):
                snap[k].append(event_ms(lambda: MS.snap_to_field(v, 0.3, *cloud, n_iter=k), 1))
        res["snap_iter_ms"] = float(np.median(snap[2]) - np.median(snap[1]))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[128, 256, 512])
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--gaussians", type=int, default=50000)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mesh_bench needs the GPU: a timing taken anywhere else says nothing")
    dev = torch.device("cuda:0")
    c = S.make_cloud(a.gaussians, seed=7)
    cloud = tuple(t.to(dev) for t in (c.xyz, c.density, c.scales, c.rotations))
    rows = []
    for n in a.sizes:
        for name, make in (("sphere", sphere), ("phantom", phantom)):
            vol, level = make(n, dev)
            rows.append(bench_volume(name, vol, level, a.rounds, a.reps, dev, cloud))
            del vol
            torch.cuda.empty_cache()
    print("%-8s %5s %10s %10s | %9s %8s | %9s %8s | %10s | %9s" % ("volume", "n", "verts", "tris", "count ms", "GB/s", "fill ms",
                                                                    "GB/s", "whole ms", "snap ms"))
    for r in rows:
        print("%-8s %5d %10d %10d | %9.4f %8.0f | %9.4f %8.0f | %10.3f | %9.3f" % (
            r["volume"], r["n"], r["verts"], r["tris"], r["count_ms"], r["count_gbps"], r["fill_ms"], r["fill_gbps"],
            r["isosurface_ms"], r.get("snap_iter_ms", float("nan"))))
    print(json.dumps({"rounds": a.rounds, "reps": a.reps, "gaussians": a.gaussians, "rows": rows}))


if __name__ == "__main__":
    main()
