"""GPU: the batched densification statistics (r2_densify_stats_batch, densify.densification_stats_batch) bit for bit against V
sequential single-view calls, with and without a gradient scale."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _inputs(V, P, gpu):
    """Random radii (a third of them 0; of several views one all 0), gradients well inside the normal range, non-zero
    statistics."""
    g = torch.Generator().manual_seed(17 * V + P)
    radii = torch.randint(1, 40, (V, P), generator=g, dtype=torch.int32)
    radii[torch.rand(V, P, generator=g) < 1.0 / 3.0] = 0
    if V > 1:
        radii[V // 2] = 0
    sign = torch.where(torch.rand(V, P, 3, generator=g) < 0.5, -1.0, 1.0)
    grad = sign * (10.0 ** (-6.0 + 5.0 * torch.rand(V, P, 3, generator=g)))      # 1e-6 .. 1e-1 in magnitude
    stats = (torch.randint(0, 30, (P,), generator=g).float(), torch.rand(P, 1, generator=g) * 1e-3,
             torch.randint(0, 50, (P, 1), generator=g).float())
    return radii.to(gpu), grad.float().contiguous().to(gpu), [t.to(gpu) for t in stats]


@pytest.mark.parametrize("P", [0, 1, 65, 300_000])
@pytest.mark.parametrize("V", [1, 3, 8])
def test_batch_equals_sequential_calls(V, P, gpu):
    from r2_gaussian_amd.densify import densification_stats, densification_stats_batch
    radii, grad, stats = _inputs(V, P, gpu)
    for scale in (1.0, 4.0):
        want = [t.clone() for t in stats]
        for v in range(V):
            densification_stats(radii[v], (scale * grad[v]).contiguous(), *want)
        got = [t.clone() for t in stats]
        densification_stats_batch(radii, grad, *got, grad_scale=scale)
        torch.cuda.synchronize()
        for name, a, b, before in zip(("max_radii2D", "grad_accum", "denom"), got, want, stats):
            assert torch.equal(a, b), (name, scale)
            if P > 1:
                assert not torch.equal(a, before), name      # the call did something
        unseen = (radii <= 0).all(0)              # Gaussians no view saw keep their statistics
        for a, before in zip(got, stats):
            assert torch.equal(a[unseen], before[unseen])


def test_model_method_takes_both_layouts(gpu):
    from r2_gaussian_amd.gaussians import GaussianModel
    V, P = 3, 500
    radii, grad, stats = _inputs(V, P, gpu)
    models = []
    for _ in range(2):
        m = GaussianModel(device=gpu)
        g = torch.Generator().manual_seed(0)
        m._set(torch.rand(P, 3, generator=g), torch.rand(P, 1, generator=g), torch.rand(P, 3, generator=g) - 3.0,
               torch.rand(P, 4, generator=g) + 0.1)
        m.max_radii2D, m.xyz_gradient_accum, m.denom = (t.clone() for t in stats)
        models.append(m)
    for v in range(V):
        models[0].add_densification_stats(radii[v], grad[v].contiguous())
    models[1].add_densification_stats(radii, grad)
    torch.cuda.synchronize()
    for n in ("max_radii2D", "xyz_gradient_accum", "denom"):
        assert torch.equal(getattr(models[0], n), getattr(models[1], n)), n


def test_library_rejects_invalid_arguments(gpu):
    from r2_gaussian_amd import _lib
    L = _lib.lib()
    radii, grad, stats = _inputs(2, 65, gpu)
    ptrs = [radii.data_ptr(), grad.data_ptr(), 1.0] + [t.data_ptr() for t in stats]
    assert L.r2_densify_stats_batch(65, 2, *ptrs, None) == 0
    assert L.r2_densify_stats_batch(0, 2, None, None, 1.0, None, None, None, None) == 0      # P == 0 enqueues nothing
    assert L.r2_densify_stats_batch(-1, 2, *ptrs, None) == _lib.R2_ERR_INVALID
    assert L.r2_densify_stats_batch(65, 0, *ptrs, None) == _lib.R2_ERR_INVALID
    for k in (0, 1, 3, 4, 5):
        bad = list(ptrs)
        bad[k] = None
        assert L.r2_densify_stats_batch(65, 2, *bad, None) == _lib.R2_ERR_INVALID, k
        assert b"r2_densify_stats_batch" in L.r2_last_error()
    torch.cuda.synchronize()
