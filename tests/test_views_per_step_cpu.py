"""CPU: the host side of several views per optimiser step -- the trainer's flag, its view picker against mini_trainer's pop
loop, the C ABI's three new entry points in the header and the ctypes table, and image_loss_batch's shape checks (which come
before anything touches the library or a device)."""
import random

import pytest
import torch

from tests.test_abi_cpu import declared_symbols


def test_parser_knows_views_per_step():
    from r2_gaussian_amd import train as TR
    ap = TR.build_parser()
    assert ap.parse_args(["-s", "x"]).views_per_step == 1
    assert ap.parse_args(["-s", "x", "--views_per_step", "8"]).views_per_step == 8


def _mini_trainer_sequence(n_views, W, steps, seed):
    """tests/mini_trainer.py:445-449, the loop itself."""
    pyrng = random.Random(seed)
    stack, out = [], []
    for _ in range(steps):
        step_views = []
        for _ in range(W):
            if not stack:
                stack = list(range(n_views))
            step_views.append(stack.pop(pyrng.randint(0, len(stack) - 1)))
        out.append(step_views)
    return out


@pytest.mark.parametrize("W", [1, 3, 8])
def test_view_picker_draws_mini_trainers_sequence(W):
    from r2_gaussian_amd import train as TR
    n_views, steps, seed = 50, 40, 5
    want = _mini_trainer_sequence(n_views, W, steps, seed)
    rng, stack, got = random.Random(seed), [], []
    straddles = 0
    for _ in range(steps):
        before = len(stack)
        got.append(TR.pick_views(stack, n_views, W, rng))
        straddles += 0 < before < W
    assert got == want
    assert all(len(g) == W for g in got)
    if W in (3, 8):
        assert straddles > 0                  # 50 is a multiple of neither: some steps take views from both sides of a refill
    flat = [v for g in got for v in g]
    first = flat[:n_views]
    assert len(set(first)) == len(first) and set(first) <= set(range(n_views))   # no view comes again before the refill


def test_new_entry_points_are_declared_and_bound():
    from r2_gaussian_amd import _lib
    names = ("r2_loss_l1_ssim_batch", "r2_loss_l1_ssim_batch_scratch_floats", "r2_densify_stats_batch")
    for n in names:
        assert n in declared_symbols(), n
        assert n in _lib.exported_symbols(), n
    assert len(_lib._SIGNATURES["r2_loss_l1_ssim_batch"][1]) == 11
    assert len(_lib._SIGNATURES["r2_densify_stats_batch"][1]) == 9
    src = open(__import__("tests.test_abi_cpu", fromlist=["HEADER"]).HEADER).read()
    assert "#define R2_LOSS_BATCH_CHUNK %d" % _lib.R2_LOSS_BATCH_CHUNK in src


def test_image_loss_batch_rejects_bad_shapes_before_the_library(monkeypatch):
    from r2_gaussian_amd import _lib, losses

    def no_library():
        raise AssertionError("the library was touched before the shapes were checked")
    monkeypatch.setattr(_lib, "lib", no_library)
    img = torch.zeros(3, 8, 10)
    ok = [torch.zeros(8, 10), torch.zeros(1, 8, 10), torch.zeros(8, 10)]
    bad = [
        (img, []),                                                  # empty list
        (img, ok[:2]),                                              # len(gts) != V
        (img, [ok[0], ok[1], torch.zeros(8, 11)]),                  # a ground truth of another size
        (img, [ok[0], ok[1], torch.zeros(2, 8, 10)]),               # [2, H, W] is not one image
        (img, torch.zeros(2, 8, 10)),                               # a [V', H, W] tensor with V' != V
        (img, torch.zeros(3, 10, 8)),
        (torch.zeros(8, 10), [ok[0]]),                              # images must be [V, H, W]
        (torch.zeros(0, 8, 10), []),                                # V = 0
    ]
    for images, gts in bad:
        with pytest.raises(ValueError):
            losses.image_loss_batch(images, gts)
    # good shapes on CPU tensors get past the shape checks and are refused as such: there is no CPU fallback
    monkeypatch.undo()
    with pytest.raises(_lib.R2HipError):
        losses.image_loss_batch(img, ok)
