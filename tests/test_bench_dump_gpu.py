"""bench.py --dump-outputs on the HIP path: the names, shapes and dtype of what it writes, and that the arrays are what the last
timed step computed -- the same view rendered and differentiated through the drop-in surface in this process."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from r2_gaussian_amd import scene as S

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_dump_outputs_are_the_last_timed_step(gpu, tmp_path):
    from r2_gaussian_amd import GaussianRasterizationSettings, GaussianRasterizer
    P, HW, NV, W, K = 2000, 64, 4, 2, 5
    d = str(tmp_path / "dump")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(K), "--warmup", str(W),
                        "--headline-only", "--gaussians", str(P), "--detector", str(HW), "--views", str(NV),
                        "--dump-outputs", d], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert line["steps"] == K and line["timing"]["timed_steps"] == K
    out = line["outputs"]
    k_last = W + min(10, K) + K - 1   # warm-up, the untimed instrumented pre-pass, then the timed steps
    assert out["step"] == k_last and out["view"] == k_last % NV
    shapes = {"image": [1, HW, HW], "radii": [P], "grad_means3D": [P, 3], "grad_means2D": [P, 3], "grad_opacities": [P, 1],
              "grad_scales": [P, 3], "grad_rotations": [P, 4]}
    assert out["arrays"] == shapes
    got = {n: np.load(os.path.join(d, n + ".npy")) for n in shapes}
    for n, a in got.items():
        assert a.dtype == np.float32 and list(a.shape) == shapes[n], n

    # the same inputs as bench.py (seed-0 cloud, its view set, its fixed dL/dpix), view out["view"], through the drop-in classes
    c = S.make_cloud(P, seed=0)
    v = S.make_views(NV, (HW, HW))[out["view"]]
    xyz, dens, scal, rot = (t.to(gpu).requires_grad_(True) for t in (c.xyz, c.density, c.scales, c.rotations))
    m2d = torch.zeros_like(xyz, requires_grad=True)
    rs = GaussianRasterizationSettings(
        image_height=HW, image_width=HW, tanfovx=v.tanfovx, tanfovy=v.tanfovy, scale_modifier=1.0,
        viewmatrix=v.world_view_transform.to(gpu), projmatrix=v.full_proj_transform.to(gpu), campos=v.camera_center.to(gpu),
        prefiltered=False, mode=v.mode, debug=False)
    img, radii = GaussianRasterizer(rs)(means3D=xyz, means2D=m2d, opacities=dens, scales=scal, rotations=rot)
    img.backward(S.make_pixel_grad(HW, HW).to(gpu))
    torch.cuda.synchronize()
    want = {"image": img, "radii": radii, "grad_means3D": xyz.grad, "grad_means2D": m2d.grad, "grad_opacities": dens.grad,
            "grad_scales": scal.grad, "grad_rotations": rot.grad}
    assert float(img.abs().max()) > 0 and bool((radii > 0).any())
    for n, t in want.items():
        w = t.detach().float().cpu().numpy()
        # same kernels, same inputs; only the order of float atomic sums in the backward may differ between the two processes
        tol = 1e-5 * max(float(np.abs(w).max()), 1e-30)
        assert np.abs(got[n] - w).max() <= tol, n
