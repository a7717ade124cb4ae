"""One sha256 per output tensor of every public entry of the exact operators, on the small scenes of the tests' reference
modules (tests/gaussian_*_ref.py).  The family is compiled with -ffp-contract=off and sums in a fixed order, so two builds
that compute the same thing print the same JSON, bit for bit, on the same machine and compiler: run it against both and
compare the files.  (R2HIP_LIB selects the library, see r2_gaussian_amd/_lib.py.)

    python scripts/exact_ops_digest.py [--out digest.json]

Entries: project_gaussians_rays forward, parameter backward and ray backward; query_points forward and backward (parameters
and points); integrate_rays with method "blocks" and "leaves", forward and backward (parameters and rays); fisher_diagonal_rays
with and without weights; field_variance; projection_variance_rays.  Not a test and not a gate; no digest file is committed,
the bits also belong to the compiler version.
"""
import argparse
import hashlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from r2_gaussian_amd import uncertainty as U                                                   # noqa: E402
from r2_gaussian_amd.field import query_points                                                 # noqa: E402
from r2_gaussian_amd.gaussian_projector import integrate_rays, project_gaussians_rays          # noqa: E402
from tests import gaussian_bundle_ref as RB                                                    # noqa: E402
from tests import gaussian_field_ref as RF                                                     # noqa: E402
from tests import gaussian_fisher_ref as RU                                                    # noqa: E402
from tests import gaussian_leaves_ref as RL                                                    # noqa: E402

GROUPS = ("xyz", "density", "scaling", "rotation")


def sha(t):
    a = np.ascontiguousarray(t.detach().cpu().numpy())
    return hashlib.sha256(str(a.shape).encode() + a.tobytes()).hexdigest()


def leaves(cloud, dev):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(dev).requires_grad_(True) for a in cloud]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="", help="also write the digests to this JSON file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("exact_ops_digest.py runs the kernels: no GPU visible")
    dev = torch.device("cuda:0")
    res = {}

    for name in RU.PROJ_SCENES:   # the projector's scenes, the ray backward's wide one and the isotropic one
        sc = RU.proj_scene(name)
        H, W, cone, mod = sc["H"], sc["W"], sc["cone"], sc["mod"]
        lv = leaves(sc["cloud"], dev)
        rays = torch.from_numpy(sc["rays"]).to(dev).requires_grad_(True)
        img = project_gaussians_rays(rays, cone, H, W, *lv, scale_modifier=mod)
        grads = torch.autograd.grad(img, lv + [rays], torch.from_numpy(sc["G"]).to(dev))
        key = "project/" + name
        res[key + "/image"] = sha(img)
        for g, t in zip(GROUPS + ("rays",), grads):
            res[key + "/d_" + g] = sha(t)
        cloud = [t.detach() for t in lv]
        wts = torch.from_numpy(RU.scene_weights(rays.shape[0], H, W)).to(dev)
        for tag, w in (("fisher", None), ("fisher_weighted", wts)):
            F = U.fisher_diagonal_rays(rays.detach(), cone, H, W, *cloud, weights=w, scale_modifier=mod)
            for g, t in zip(GROUPS, F):
                res["%s/%s/%s" % (tag, name, g)] = sha(t)
        var = RU.scene_variances(cloud[0].shape[0])
        var = tuple(torch.from_numpy(var[g]).to(dev) for g in GROUPS)
        pv = U.projection_variance_rays(rays.detach(), cone, H, W, *cloud, var, scale_modifier=mod)
        res["projection_variance/" + name] = sha(pv)

    for name in RF.SCENES:
        sc = RF.scene(name)
        lv = leaves(sc["cloud"], dev)
        pts = torch.from_numpy(sc["points"]).to(dev).requires_grad_(True)
        val = query_points(pts, *lv, scale_modifier=sc["mod"])
        grads = torch.autograd.grad(val, lv + [pts], torch.from_numpy(sc["G"]).to(dev).reshape(val.shape))
        key = "query/" + name
        res[key + "/value"] = sha(val)
        for g, t in zip(GROUPS + ("points",), grads):
            res[key + "/d_" + g] = sha(t)
        var = RU.scene_variances(lv[0].shape[0])
        var = tuple(torch.from_numpy(var[g]).to(dev) for g in GROUPS)
        fv = U.field_variance(pts.detach(), *[t.detach() for t in lv], var, scale_modifier=sc["mod"])
        res["field_variance/" + name] = sha(fv)

    for ref, method in ((RB, "blocks"), (RB, "leaves"), (RL, "blocks"), (RL, "leaves")):   # both scene sets through both methods
        for name in ref.SCENES:
            sc = ref.scene(name)
            lv = leaves(sc["cloud"], dev)
            o = torch.from_numpy(sc["origins"]).to(dev).requires_grad_(True)
            d = torch.from_numpy(sc["directions"]).to(dev).requires_grad_(True)
            val = integrate_rays(o, d, *lv, scale_modifier=sc["mod"], half_line=sc["half_line"], method=method)
            grads = torch.autograd.grad(val, lv + [o, d], torch.from_numpy(sc["G"]).to(dev).reshape(val.shape))
            key = "integrate_%s/%s" % (method, name)
            res[key + "/value"] = sha(val)
            for g, t in zip(GROUPS + ("origins", "directions"), grads):
                res[key + "/d_" + g] = sha(t)

    torch.cuda.synchronize()
    text = json.dumps(res, indent=1, sort_keys=True)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
