"""Isosurfaces as triangle meshes: of a volume (``isosurface``: marching tetrahedra on the kernels of csrc/isosurface.hip,
``r2_isosurface_count`` / ``r2_isosurface_fill``; include/r2hip.h states the contract) and of the Gaussian model's continuous
density (``model_isosurface``: the field on a grid by ``field.query_points``, its isosurface, and ``snap_to_field``, which moves
the vertices onto the model's own level set by Newton steps along the exact gradient, so that the mesh no longer depends on the
voxel size of the grid it was found on).  ``mesh_area`` / ``mesh_volume`` measure a mesh, ``write_ply`` / ``write_stl`` write it.

The reference builds its meshes with ``skimage.measure.marching_cubes`` and Open3D (``plot_utils.create_vol_mesh`` behind
``visualize_scene.py --mc_thresh``).  Its vertices are ``idx sVoxel / nVoxel - sVoxel / 2 + center``: voxel idx at the LOWER
CORNER of its cell.  Here voxel idx sits where the voxelizer samples it (``field.voxel_centres``), half a voxel further.

    python -m r2_gaussian_amd.mesh --volume vol.npy | --model point_cloud.pickle  [--level 0.5] [--scanner cfg.yml | --meta
        meta_data.json] [--closed] [--snap] --out mesh.ply | mesh.stl
"""
import struct

import numpy as np
import torch

from . import _lib
from ._boundary import _F32, call, f32c, require_gpu, workspace
from .field import query_points, voxel_centres


def _frame(n, center, sVoxel):
    """(origin, spacing) of the lattice in float64: voxel idx at center - sVoxel / 2 + (idx + 0.5) sVoxel / nVoxel."""
    if sVoxel is None:
        if center is not None:
            raise ValueError("center without sVoxel: the output is then in index coordinates")
        return [0.0] * 3, [1.0] * 3
    center = [0.0] * 3 if center is None else [float(c) for c in center]
    sVoxel = [float(s) for s in sVoxel]
    if len(center) != 3 or len(sVoxel) != 3 or not all(s > 0 for s in sVoxel):
        raise ValueError("center and sVoxel must have three entries each, sVoxel positive")
    d = [s / k for s, k in zip(sVoxel, n)]
    return [c - s / 2 + 0.5 * dd for c, s, dd in zip(center, sVoxel, d)], d


def isosurface(vol, level, center=None, sVoxel=None, normals=True, closed=False, fill=0.0):
    """The surface {vol = level} of ``vol`` [nx,ny,nz] (GPU) -> (verts [Nv,3] float32, faces [Nf,3] int32, normals [Nv,3]
    float32 or None) on the volume's device.  Marching tetrahedra: watertight, no ambiguous cases; a voxel is inside iff
    vol >= level, the faces run counter-clockwise seen from the low side, and the normals (minus the normalised lattice
    gradient, central differences interpolated along the edge) point the same way, from inside to outside.
    sVoxel None: index coordinates (voxel idx at idx).  Otherwise voxel idx sits at ``field.voxel_centres``' position,
    center - sVoxel / 2 + (idx + 0.5) sVoxel / nVoxel (center defaults to the origin): half a voxel further than the
    reference's ``create_vol_mesh`` puts it, which omits the half voxel.
    closed: the volume is padded by one voxel of ``fill`` (< level, else ValueError) on every side, so that a surface that
    reaches the border is capped there.  A NaN, an infinity or a value above 1e38 in magnitude raises ValueError.
    One host read (the counts), as ``gaussian_projector.plan_projection`` has."""
    if not isinstance(vol, torch.Tensor) or vol.dim() != 3 or min(vol.shape) < 1:
        raise ValueError("vol must be a tensor [nx,ny,nz], got %s" % (tuple(getattr(vol, "shape", ())),))
    require_gpu(vol, "vol")
    level = float(level)
    if not np.isfinite(level):
        raise ValueError("level must be finite, got %r" % level)
    origin, spacing = _frame(vol.shape, center, sVoxel)
    v = f32c(vol.detach())
    if closed:
        if not float(fill) < float(np.float32(level)):
            raise ValueError("closed: fill must be below level, got fill %r and level %r" % (fill, level))
        v = torch.nn.functional.pad(v, (1, 1, 1, 1, 1, 1), value=float(fill))
        origin = [o - d for o, d in zip(origin, spacing)]
    nx, ny, nz = (int(n) for n in v.shape)
    if nx * ny * nz >= (1 << 31):
        raise ValueError("fewer than 2^31 lattice points, got %d x %d x %d" % (nx, ny, nz))
    dev = v.device
    ws = workspace(_lib.lib().r2_isosurface_workspace_bytes(nx, ny, nz), dev, at_least=1)
    counts = torch.empty((3,), dtype=torch.int64, device=dev)
    call("r2_isosurface_count", dev, nx, ny, nz, v, level, ws, ws.numel(), counts)
    nv, nt, bad = (int(c) for c in counts.cpu())   # the one host read
    if bad:
        raise ValueError("the volume holds %d invalid values (NaN, infinite or above 1e38 in magnitude)" % bad)
    if nv >= (1 << 31) or nt >= (1 << 31):
        raise ValueError("the surface has %d vertices and %d triangles; fewer than 2^31 of each are supported" % (nv, nt))
    verts = torch.empty((nv, 3), dtype=_F32, device=dev)
    faces = torch.empty((nt, 3), dtype=torch.int32, device=dev)
    nrm = torch.empty((nv, 3), dtype=_F32, device=dev) if normals else None
    call("r2_isosurface_fill", dev, nx, ny, nz, v, level, *origin, *spacing, ws, ws.numel(), nv, nt,
         verts if nv else None, nrm if nv else None, faces if nt else None)
    return verts, faces, nrm


def _field_and_gradient(points, level, xyz, density, scaling, rotation, scale_modifier):
    p = points.detach().requires_grad_(True)
    with torch.enable_grad():
        s = query_points(p, xyz.detach(), density.detach(), scaling.detach(), rotation.detach(), scale_modifier)
        g, = torch.autograd.grad(s.sum(), p)
    return s.detach() - level, g


def snap_to_field(verts, level, xyz, density, scaling, rotation, n_iter=4, max_step=None, scale_modifier=1.0):
    """Moves ``verts`` [N,3] (GPU) onto the level set {sigma = level} of the Gaussian model's continuous density by ``n_iter``
    Newton steps along the gradient, v <- v - (sigma(v) - level) g / |g|^2, sigma and g = grad sigma from ``field.query_points``
    and its exact gradient in the points.  max_step (None: no limit): the length every step is clipped to; half a voxel of
    the grid the vertices were found on keeps a vertex in the neighbourhood of its edge.  A vertex whose |g| is zero stays
    where it is.  -> (verts [N,3], normals [N,3]: -g / |g| at the final positions, zeros where |g| = 0)."""
    if not isinstance(verts, torch.Tensor) or verts.dim() != 2 or verts.shape[1] != 3:
        raise ValueError("verts must be a tensor [N,3], got %s" % (tuple(getattr(verts, "shape", ())),))
    require_gpu(verts, "verts")
    if int(n_iter) < 0 or (max_step is not None and not float(max_step) > 0):
        raise ValueError("n_iter must be >= 0 and max_step positive, got %r and %r" % (n_iter, max_step))
    level = float(level)
    v = f32c(verts.detach()).clone()
    if v.shape[0] == 0:
        return v, torch.zeros_like(v)
    cloud = (xyz, density, scaling, rotation, float(scale_modifier))
    for _ in range(int(n_iter)):
        r, g = _field_and_gradient(v, level, *cloud)
        g2 = (g * g).sum(1, keepdim=True)
        step = torch.where(g2 > 0, r[:, None] * g / torch.where(g2 > 0, g2, torch.ones_like(g2)), torch.zeros_like(g))
        if max_step is not None:
            ln = step.norm(dim=1, keepdim=True)
            step = step * torch.clamp(float(max_step) / torch.where(ln > 0, ln, torch.ones_like(ln)), max=1.0)
        v = v - step
    _, g = _field_and_gradient(v, level, *cloud)
    n = g.norm(dim=1, keepdim=True)
    return v, torch.where(n > 0, -g / torch.where(n > 0, n, torch.ones_like(n)), torch.zeros_like(g))


def model_isosurface(xyz, density, scaling, rotation, level, center, nVoxel, sVoxel, snap=True, closed=True):
    """The isosurface of the model's continuous density at ``level``: the field at ``field.voxel_centres(center, nVoxel,
    sVoxel)`` by ``query_points``, ``isosurface`` of that grid (closed: capped at the grid's border, fill 0), and with ``snap``
    the vertices moved onto the field's own level set (``snap_to_field``, steps of at most half a voxel) with the field's
    gradient as normals.  The cap of a closed surface lies outside the grid, where the field is not the level: its vertices
    move too, by at most half a voxel per step.  -> (verts, faces, normals)."""
    require_gpu(xyz, "xyz")
    pts = voxel_centres(center, nVoxel, sVoxel, xyz.device)
    with torch.no_grad():
        vol = query_points(pts, xyz.detach(), density.detach(), scaling.detach(), rotation.detach())
    verts, faces, nrm = isosurface(vol, level, center, sVoxel, normals=True, closed=closed)
    if snap:
        half = 0.5 * min(float(s) / int(n) for s, n in zip(sVoxel, nVoxel))
        verts, nrm = snap_to_field(verts, level, xyz, density, scaling, rotation, max_step=half)
    return verts, faces, nrm


def _corners(verts, faces):
    v = verts.detach().to(torch.float64)
    f = faces.detach().to(torch.int64)
    if v.dim() != 2 or v.shape[1] != 3 or f.dim() != 2 or f.shape[1] != 3:
        raise ValueError("verts must be [Nv,3] and faces [Nf,3], got %s and %s" % (tuple(v.shape), tuple(f.shape)))
    return v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]


def mesh_area(verts, faces):
    """The area of the mesh: a float64 reduction on the mesh's device -> a 0-d float64 tensor."""
    a, b, c = _corners(verts, faces)
    return 0.5 * torch.linalg.cross(b - a, c - a).norm(dim=1).sum()


def mesh_volume(verts, faces):
    """The signed volume a closed mesh encloses, by the divergence theorem (sum of a . (b x c) / 6): positive when the faces run
    counter-clockwise seen from outside, as ``isosurface`` orients them.  float64, on the mesh's device."""
    a, b, c = _corners(verts, faces)
    return (a * torch.linalg.cross(b, c)).sum() / 6.0


def _host(t, dtype):
    return np.ascontiguousarray((t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)).astype(dtype))


def write_ply(path, verts, faces, normals=None):
    """Binary little-endian PLY: vertices x y z (float32), with ``normals`` nx ny nz, faces as lists of three int32."""
    v, f = _host(verts, "<f4").reshape(-1, 3), _host(faces, "<i4").reshape(-1, 3)
    props = ["x", "y", "z"]
    if normals is not None:
        n = _host(normals, "<f4").reshape(-1, 3)
        if n.shape != v.shape:
            raise ValueError("normals are %s, vertices %s" % (n.shape, v.shape))
        v = np.concatenate([v, n], 1)
        props += ["nx", "ny", "nz"]
    head = ["ply", "format binary_little_endian 1.0", "comment r2_gaussian_amd.mesh", "element vertex %d" % v.shape[0]]
    head += ["property float %s" % p for p in props]
    head += ["element face %d" % f.shape[0], "property list uchar int vertex_indices", "end_header"]
    rec = np.empty(f.shape[0], dtype=[("n", "u1"), ("v", "<i4", (3,))])
    rec["n"] = 3
    rec["v"] = f
    with open(path, "wb") as fh:
        fh.write(("\n".join(head) + "\n").encode("ascii"))
        fh.write(np.ascontiguousarray(v, "<f4").tobytes())
        fh.write(rec.tobytes())


def write_stl(path, verts, faces):
    """Binary STL: per triangle its float32 unit normal (zeros for a degenerate one) and its three corners."""
    v, f = _host(verts, "<f4").reshape(-1, 3), _host(faces, "<i4").reshape(-1, 3)
    tri = v[f]                                         # [Nf,3,3]
    n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]).astype(np.float64)
    ln = np.linalg.norm(n, axis=1, keepdims=True)
    n = np.where(ln > 0, n / np.where(ln > 0, ln, 1.0), 0.0).astype("<f4")
    rec = np.zeros(f.shape[0], dtype=[("n", "<f4", (3,)), ("v", "<f4", (3, 3)), ("attr", "<u2")])
    rec["n"] = n
    rec["v"] = tri
    with open(path, "wb") as fh:
        fh.write(b"r2_gaussian_amd.mesh".ljust(80, b" "))
        fh.write(struct.pack("<I", f.shape[0]))
        fh.write(rec.tobytes())


def write_mesh(path, verts, faces, normals=None):
    if path.lower().endswith(".stl"):
        write_stl(path, verts, faces)
    elif path.lower().endswith(".ply"):
        write_ply(path, verts, faces, normals)
    else:
        raise ValueError("the mesh file must end in .ply or .stl, got %r" % path)


def _extent(args):
    """(center, sVoxel, nVoxel) of the raw scanner config of --scanner (YAML) or --meta (meta_data.json), or None."""
    if args.scanner:
        import yaml
        with open(args.scanner, "r") as f:
            cfg = yaml.safe_load(f)
    elif args.meta:
        import json
        with open(args.meta, "r", encoding="utf-8") as f:
            cfg = json.load(f)["scanner"]
    else:
        return None
    return [float(c) for c in cfg["offOrigin"]], [float(s) for s in cfg["sVoxel"]], [int(n) for n in cfg["nVoxel"]]


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(description="Isosurface of a volume, or of a Gaussian model's density, as a triangle mesh")
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument("--volume", type=str, help="a volume [nx,ny,nz] as .npy")
    src.add_argument("--model", type=str, help="a model file (point_cloud.pickle, raw parameters) as model_io reads it")
    ap.add_argument("--level", type=float, default=0.5, help="the level (default 0.5: the reference's --mc_thresh default)")
    ext = ap.add_mutually_exclusive_group()
    ext.add_argument("--scanner", type=str, help="scanner configuration (YAML): nVoxel, sVoxel, offOrigin give the extent")
    ext.add_argument("--meta", type=str, help="a case's meta_data.json: its scanner configuration gives the extent")
    ap.add_argument("--closed", action="store_true", help="cap the surface where it reaches the border of the grid")
    ap.add_argument("--snap", action="store_true", help="--model: move the vertices onto the continuous field's level set")
    ap.add_argument("--out", type=str, required=True, help="mesh.ply or mesh.stl")
    ap.add_argument("--device", type=str, default="cuda")
    args = ap.parse_args(argv)
    if not args.out.lower().endswith((".ply", ".stl")):
        ap.error("--out must end in .ply or .stl")
    extent = _extent(args)
    if args.volume:
        if args.snap:
            ap.error("--snap needs --model: a volume has no continuous field")
        vol = torch.from_numpy(np.load(args.volume).astype(np.float32)).to(args.device)
        if extent is not None and list(vol.shape) != extent[2]:
            ap.error("the volume is %s, the scanner configuration's nVoxel %s" % (list(vol.shape), extent[2]))
        center, sVoxel = (None, None) if extent is None else extent[:2]
        verts, faces, nrm = isosurface(vol, args.level, center, sVoxel, closed=args.closed)
    else:
        if extent is None:
            ap.error("--model needs --scanner or --meta for the grid")
        from . import model_io
        # a trained model lives in scene units (dataset_readers.py:62-76): the raw configuration times 2 / max(sVoxel)
        scale = 2.0 / max(extent[1])
        center, sVoxel = [c * scale for c in extent[0]], [s * scale for s in extent[1]]
        x, d, s, r = model_io.activate(model_io.load_point_cloud(args.model, device=args.device))
        verts, faces, nrm = model_isosurface(x, d, s, r, args.level, center, extent[2], sVoxel, snap=args.snap, closed=args.closed)
    write_mesh(args.out, verts, faces, nrm)
    print("%s: %d vertices, %d triangles, area %.6g, volume %.6g" % (args.out, verts.shape[0], faces.shape[0],
                                                                      float(mesh_area(verts, faces)), float(mesh_volume(verts, faces))))


if __name__ == "__main__":
    main()
