"""CPU, world_size 2 over gloo: the view-sharded data-parallel exchange (r2_gaussian_amd/dist.py).  The N>1 path of
bench.py / training uses exactly these functions with backend "nccl" (= RCCL) on GPUs."""
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from r2_gaussian_amd import dist as D


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, q):
    try:
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        dist.init_process_group("gloo", rank=rank, world_size=world)
        P = 257
        g = torch.Generator().manual_seed(100 + rank)
        grads = [torch.randn(P, w, generator=g) for w in (3, 1, 3, 4)]
        flat = D.pack_grads(*grads)
        assert flat.shape == (P, D.GRAD_WIDTH)
        for a, b in zip(D.unpack_grads(flat), grads):
            assert torch.equal(a, b)
        # expected mean over ranks, computed locally from the known seeds
        want = torch.zeros(P, D.GRAD_WIDTH)
        for r in range(world):
            gr = torch.Generator().manual_seed(100 + r)
            want += D.pack_grads(*[torch.randn(P, w, generator=gr) for w in (3, 1, 3, 4)])
        D.allreduce_grads(flat, average=True)
        assert torch.allclose(flat, want / world, atol=1e-6)
        # parameter-level helper writes the reduced gradients back
        params = [torch.zeros(P, w, requires_grad=True) for w in (3, 1, 3, 4)]
        for p, g_ in zip(params, grads):
            p.grad = g_.clone()
        D.allreduce_param_grads(params, average=False)
        assert torch.allclose(D.pack_grads(*(p.grad for p in params)), want, atol=1e-5)
        # densification statistics: sums and max
        gn = torch.full((P,), float(rank + 1))
        dn = (torch.arange(P) % (rank + 2) == 0).float()
        rad = torch.arange(P, dtype=torch.int32) * (rank + 1)
        s_gn, s_dn, m_rad = D.allreduce_densify_stats(gn, dn, rad)
        assert torch.equal(s_gn, torch.full((P,), float(sum(range(1, world + 1)))))
        assert torch.equal(s_dn, sum((torch.arange(P) % (r + 2) == 0).float() for r in range(world)))
        assert torch.equal(m_rad, torch.arange(P, dtype=torch.int32) * world)
        # view sharding: ranks of one step render distinct views; over an epoch every view is visited
        n_views = 7
        mine = [D.view_for(k, n_views) for k in range(n_views)]
        allv = [None] * world
        dist.all_gather_object(allv, mine)
        for k in range(n_views):
            assert len({allv[r][k] for r in range(world)}) == world
        assert sorted(v for r in range(world) for v in allv[r]) == sorted(list(range(n_views)) * world)
        # replica check: equal tensors pass, diverged tensors raise on every rank
        D.assert_replicas_equal(torch.ones(5), "same")
        try:
            D.assert_replicas_equal(torch.ones(5) * (rank + 1), "diverged")
            q.put((rank, "divergence not detected"))
            return
        except RuntimeError:
            pass
        dist.barrier()
        dist.destroy_process_group()
        q.put((rank, "ok"))
    except Exception as e:   # surface the failure in the parent
        import traceback
        q.put((rank, "FAIL %r\n%s" % (e, traceback.format_exc())))


@pytest.mark.timeout(180)
def test_world2_gloo_exchange():
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=150) for _ in range(world)]
    for p in procs:
        p.join(30)
    assert sorted(res) == [(0, "ok"), (1, "ok")], res


def test_single_process_is_identity():
    assert D.world() == 1 and D.rank() == 0
    flat = torch.ones(4, D.GRAD_WIDTH)
    assert D.allreduce_grads(flat) is None and torch.equal(flat, torch.ones(4, D.GRAD_WIDTH))
    assert [D.view_for(k, 5, rank_=1, world_=2) for k in range(5)] == [1, 3, 0, 2, 4]


def test_voxel_slab_settings_tile_the_volume():
    """x-slab sharding of the full-volume query: whole tile layers, contiguous, covering [0, nx) exactly once; every rank keeps the
    FULL volume's settings (same centre, same voxel size: the arithmetic of the unsharded call) + its range of layers."""
    from r2_gaussian_amd import dist as D
    from r2_gaussian_amd.voxelization import GaussianVoxelizationSettings as VS
    for nx, world in ((256, 8), (256, 3), (40, 4), (8, 4), (100, 8)):
        s = VS(1.0, nx, 64, 32, 2.0, 1.0, 0.5, 0.1, -0.2, 0.3, False, False)
        cover = []
        for r in range(world):
            sub, (x0, x1) = D.slab_settings(s, r, world)
            assert x0 % 8 == 0 and (x1 % 8 == 0 or x1 == nx)
            if sub is None:
                assert x0 == x1
                continue
            cover.append((x0, x1))
            assert tuple(sub)[:12] == tuple(s), "a slab keeps the full volume's settings"
            assert sub.tile_x0 * 8 == x0 and min(sub.tile_x1 * 8, nx) == x1 and sub.tile_x1 > sub.tile_x0
        assert cover[0][0] == 0 and cover[-1][1] == nx
        assert all(a[1] == b[0] for a, b in zip(cover[:-1], cover[1:]))


def test_grad_block_detects_the_backward_layout():
    """The drop-in backward carves rotation | xyz | scaling | density adjacent out of one buffer: dist.grad_block must hand
    that block out as one flat view (in-place all-reduce, no packing copy) and refuse anything else."""
    import torch
    from r2_gaussian_amd import dist as D
    P = 37
    flat = torch.arange(25 * P, dtype=torch.float32)
    o = 0
    conic = flat.as_strided((P, 2, 2), (4, 2, 1), o); o += 4 * P
    rot = flat.as_strided((P, 4), (4, 1), o); o += 4 * P
    xyz = flat.as_strided((P, 3), (3, 1), o); o += 3 * P
    scal = flat.as_strided((P, 3), (3, 1), o); o += 3 * P
    dens = flat.as_strided((P, 1), (1, 1), o); o += P
    blk = D.grad_block(xyz, dens, scal, rot)
    assert blk is not None and blk.shape == (11 * P,)
    assert blk.data_ptr() == rot.data_ptr() and torch.equal(blk, flat[4 * P:15 * P])
    blk.mul_(2.0)   # in place: the four gradients see it
    assert torch.equal(xyz, flat.as_strided((P, 3), (3, 1), 8 * P)) and float(xyz[0, 0]) == 2.0 * (8 * P)
    # not the backward's layout: separate tensors, wrong order, non-contiguous
    assert D.grad_block(xyz.clone(), dens, scal, rot) is None
    assert D.grad_block(scal, dens, xyz, rot) is None
    assert D.grad_block(xyz, dens, scal, conic.reshape(P, 4)) is None
    # and the packed fallback still round-trips
    packed = D.pack_grads(xyz, dens, scal, rot)
    gx, gd, gs, gr = D.unpack_grads(packed)
    assert torch.equal(gx, xyz) and torch.equal(gd, dens) and torch.equal(gs, scal) and torch.equal(gr, rot)


# ------------------------------------------------------------------------------------------------ bench.py launcher
def _bench_line(out):
    import json
    lines = [l for l in out.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out[-2000:]
    return json.loads(lines[0])


@pytest.mark.timeout(300)
def test_bench_gpus_n_launches_its_own_ranks():
    """`python bench.py --gpus 2` with no launcher around it must start 2 ranks itself (one per GPU on a node; here on CPU over
    gloo with the renderer stubbed: R2_BENCH_STUB=1), report n_gpus = 2 = the size of the process group it found, and both a
    synchronous and an overlapped number.  Under a launcher whose world differs from --gpus it must refuse."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, R2_BENCH_STUB="1")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "4", "--warmup", "2",
                        "--repeats", "3", "--gaussians", "513"], env=env, capture_output=True, text=True, timeout=280)
    assert r.returncode == 0, r.stderr[-3000:]
    line = _bench_line(r.stdout)
    assert line["n_gpus"] == 2 and line["config"]["ranks_in_process_group"] == 2
    assert line["steps"] == 4 and line["timing"]["regions"] == 3 and line["overlapped"]["regions"] == 3
    assert line["value"] > 0 and line["overlapped"]["value"] > 0
    # round 5: what north_star asks of an N > 1 line -- the synchronous modes side by side with their views per step and which
    # of them `value` is; one whole data-parallel TRAINING iteration (exchange behind the TV branch); the full-volume query
    # sharded by x-slab with and without the all-gather (the stand-in voxelizer lets bench.py check the gathered slab order);
    # the exchange path in `config`
    assert line["config"]["comm_zero_copy"] in (True, False) and "parallelism" in line["config"]
    sm = line["sync_modes"]
    assert sm["value_is"] == "sync" and sm["sync"]["value"] == line["value"]
    assert sm["sync"]["views_per_rank_and_step"] == 1 and sm["sync2"]["views_per_rank_and_step"] == sm["accum2"]["views_per_rank_and_step"] == 2
    ti = line["train_iteration"]
    assert ti["unit"] == "iterations/s" and ti["value"] > 0 and ti["views_per_iteration"] == 2
    assert abs(ti["views_per_s"] - 2 * ti["value"]) < 0.02
    sh = line["voxelizer"]["sharded"]
    assert sh["gvoxel_per_s"] > 0 and sh["with_all_gather"]["gvoxel_per_s"] > 0 and sh["gather_checked"] is True
    assert sh["slab_of_rank0"] == [0, 32] and sh["volume"] == [64, 64, 64]
    # a launcher that started a different number of ranks than --gpus says: refuse
    env2 = dict(env, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
    r2 = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1"],
                        env=env2, capture_output=True, text=True, timeout=120)
    assert r2.returncode != 0 and "launcher started 1 ranks" in (r2.stderr + r2.stdout)


@pytest.mark.timeout(300)
def test_bench_steps_and_dump_outputs(tmp_path):
    """--steps K times exactly K steps (split into regions), the line carries ms_per_step, and --dump-outputs DIR writes what the
    last timed step computed as float32 .npy files -- the same arrays on a second run with the same arguments (stub renderer)."""
    import subprocess
    import sys
    import numpy as np
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, R2_BENCH_STUB="1")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    dumps = []
    for run in range(2):
        d = str(tmp_path / ("run%d" % run))
        r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "45", "--warmup", "3",
                            "--gaussians", "257", "--dump-outputs", d], env=env, capture_output=True, text=True, timeout=280)
        assert r.returncode == 0, r.stderr[-3000:]
        line = _bench_line(r.stdout)
        assert line["steps"] == 45 and line["timing"]["timed_steps"] == 45 and line["timing"]["regions"] == 2
        assert line["ms_per_step"] > 0 and line["ms_per_step"] == line["timing"]["ms_per_step"]
        assert line["outputs"]["step"] == 3 + 45 - 1 and line["outputs"]["arrays"] == {"grad_block": [257, 11]}
        a = np.load(os.path.join(d, "grad_block.npy"))
        assert a.dtype == np.float32 and a.shape == (257, 11)
        dumps.append(a)
    assert np.array_equal(dumps[0], dumps[1])
    # the stub renders step k as the k-th draw of torch.rand from a generator seeded with the rank: the dump must be the draw
    # of the last timed step (3 warm-up + 45 timed steps), not of any earlier one
    g = torch.Generator().manual_seed(0)
    for _ in range(3 + 45):
        want = torch.rand(257, 11, generator=g)
    assert np.array_equal(dumps[0], want.numpy())


def test_bench_dump_outputs_stays_within_budget(tmp_path):
    """Above 64 MB the dump is a seeded sample of every array plus its flat element indices, and stays under 64 MB."""
    import sys
    import numpy as np
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if root not in sys.path:
        sys.path.insert(0, root)
    import bench
    big = np.arange(20_000_000, dtype=np.float32).reshape(-1, 4)
    arrays = {"big": big, "image": np.ones((1, 64, 64)), "radii": np.arange(10, dtype=np.int32)}
    shapes = [bench.dump_outputs(str(tmp_path / d), arrays) for d in ("a", "b")]
    assert shapes[0] == shapes[1]
    assert sum(f.stat().st_size for f in (tmp_path / "a").iterdir()) <= bench.DUMP_BUDGET_BYTES
    v, i = np.load(str(tmp_path / "a" / "big.npy")), np.load(str(tmp_path / "a" / "big_index.npy"))
    assert v.dtype == np.float32 and i.dtype == np.float64 and 0 < v.size < big.size
    assert np.array_equal(v, big.reshape(-1)[i.astype(np.int64)])
    assert np.array_equal(i, np.load(str(tmp_path / "b" / "big_index.npy")))
    # under the budget everything is written whole, in float32
    small = bench.dump_outputs(str(tmp_path / "c"), {"radii": arrays["radii"]})
    assert small == {"radii": [10]} and np.load(str(tmp_path / "c" / "radii.npy")).dtype == np.float32


def test_bench_step_runner_sync_and_overlap_order():
    """sync: every step's reduction is waited for before the step returns.  overlap: it is waited for two steps later, before
    its buffer is rendered into again, and drain() waits for whatever is left."""
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if root not in sys.path:
        sys.path.insert(0, root)
    import bench
    log = []

    class H:
        def __init__(self, k):
            self.k = k

        def wait(self):
            log.append(("wait", self.k))

    def render(k, i):
        log.append(("render", k, i))
        return k

    def allreduce(blk):
        log.append(("reduce", blk))
        return H(blk)

    r = bench.StepRunner(render, allreduce, True, "sync")
    for k in range(3):
        r.step(k)
    r.drain()
    assert log == [("render", 0, 0), ("reduce", 0), ("wait", 0), ("render", 1, 1), ("reduce", 1), ("wait", 1),
                   ("render", 2, 0), ("reduce", 2), ("wait", 2)]
    del log[:]
    r = bench.StepRunner(render, allreduce, True, "overlap")
    for k in range(4):
        r.step(k)
    r.drain()
    assert log == [("render", 0, 0), ("reduce", 0), ("render", 1, 1), ("reduce", 1), ("wait", 0), ("render", 2, 0),
                   ("reduce", 2), ("wait", 1), ("render", 3, 1), ("reduce", 3), ("wait", 2), ("wait", 3)]
    del log[:]
    r = bench.StepRunner(render, allreduce, False, "sync")   # single GPU: no exchange at all
    r.step(0)
    r.drain()
    assert log == [("render", 0, 0)]
    # two views per rank and step, synchronous: sync2 = A's reduction started before B renders and waited for after it, then B's;
    # accum2 = B accumulates into A's block (render's third argument), ONE reduction
    del log[:]

    def render3(k, i, accumulate=False):
        log.append(("render", k, i, accumulate))
        return k

    r = bench.StepRunner(render3, allreduce, True, "sync2")
    r.step(0)
    r.step(1)
    r.drain()
    assert log == [("render", 0, 0, False), ("reduce", 0), ("render", 1, 1, False), ("wait", 0), ("reduce", 1), ("wait", 1),
                   ("render", 2, 0, False), ("reduce", 2), ("render", 3, 1, False), ("wait", 2), ("reduce", 3), ("wait", 3)]
    del log[:]
    r = bench.StepRunner(render3, allreduce, True, "accum2")
    r.step(0)
    r.drain()
    assert log == [("render", 0, 0, False), ("render", 1, 0, True), ("reduce", 1), ("wait", 1)]
    assert bench.StepRunner.VIEWS_PER_STEP["sync2"] == bench.StepRunner.VIEWS_PER_STEP["accum2"] == 2
    s = bench.summarize([0.010, 0.012, 0.011], 10, 2)
    assert s["value"] == round(10 * 2 / 0.011, 2) and s["ms_per_step"] == 1.1 and s["regions"] == 3


# ------------------------------------------------------------------------------------------------ data-parallel trainer
# SURVEY.md 8(e) "consistency": the whole training loop (tests/mini_trainer.py: render, L1 + DSSIM + TV, Adam, densify / prune)
# run view-sharded over 2 ranks with the ORACLE backend -- one view per rank and step, ONE all-reduce of the [P,11] gradient
# block, sum / max reductions of the densification statistics (r2_gaussian_amd.dist) -- must leave bit-identical models on both
# ranks after several densification rounds, identical to a single process that renders the same two views per step.
def _dp_case_and_opt():
    from tests import mini_trainer as T
    case = T.Case(detector=32, n_vol=16, n_views=8, p_gt=600, n_init=400, seed=2)
    opt = T.Opt(iterations=120, densify_from_iter=20, densify_until_iter=110, densification_interval=30, tv_vol_size=8,
                densify_grad_threshold=2.0e-5, densify_scale_threshold=0.02)
    return case, opt


def _model_signature(model):
    import hashlib
    h = hashlib.sha256()
    for n in model.NAMES:
        h.update(model.p[n].detach().cpu().numpy().tobytes())
        st = model.optimizer.state[model.p[n]]
        h.update(st["exp_avg"].cpu().numpy().tobytes())
        h.update(st["exp_avg_sq"].cpu().numpy().tobytes())
    h.update(model.max_radii2D.cpu().numpy().tobytes())
    return model.P, h.hexdigest()


def _dp_train_worker(rank, world, port, q, views_per_rank=1, exchange="accum"):
    try:
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        torch.set_num_threads(2)
        dist.init_process_group("gloo", rank=rank, world_size=world)
        from tests import mini_trainer as T
        case, opt = _dp_case_and_opt()
        out = T.train(case, opt, "oracle", eval_every=60, seed=0, views_per_step=world * views_per_rank, data_parallel=True,
                      return_model=True, views_per_rank=views_per_rank, exchange=exchange)
        sig = _model_signature(out["model"])
        dist.barrier()
        dist.destroy_process_group()
        q.put((rank, "ok", sig, out["P"], out["psnr"]))
    except Exception as e:
        import traceback
        q.put((rank, "FAIL %r\n%s" % (e, traceback.format_exc()), None, None, None))


@pytest.mark.timeout(600)
def test_data_parallel_trainer_world2_equals_single_process():
    from tests import mini_trainer as T
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_dp_train_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    # meanwhile: the single process that renders both views of every step itself (with the workers' thread count: the
    # oracle's float accumulation -- like the reference's atomics -- associates by OpenMP thread, torch.set_num_threads sets it)
    case, opt = _dp_case_and_opt()
    nthreads = torch.get_num_threads()
    torch.set_num_threads(2)
    try:
        ref = T.train(case, opt, "oracle", eval_every=60, seed=0, views_per_step=world, return_model=True)
    finally:
        torch.set_num_threads(nthreads)
    ref_sig = _model_signature(ref["model"])
    res = sorted(q.get(timeout=500) for _ in range(world))
    for p in procs:
        p.join(30)
    assert [r[1] for r in res] == ["ok", "ok"], res
    assert res[0][2] == res[1][2], "the two ranks hold different models"
    assert len(set(ref["P"])) >= 3, ref["P"]                       # the run went through densification rounds that changed P
    assert res[0][3] == ref["P"] and res[0][2] == ref_sig, (res[0][3], ref["P"])   # bit-identical to the single-process run
    assert res[0][4] == ref["psnr"]


@pytest.mark.timeout(900)
@pytest.mark.parametrize("exchange", ["accum", "sync2"])
def test_data_parallel_two_views_per_rank_world2_equals_single_process(exchange):
    """synchronous data parallelism that hides (sync2) or halves (accum) its exchange -- every rank renders TWO
    views per optimiser step, parameters update once per step, no stale gradients.  World 2 over gloo with the oracle backend,
    three densification rounds: both ranks bit-identical, and equal to ONE process that renders the same four views per step
    and adds their gradient blocks with the same association (mini_trainer's virtual ranks)."""
    from tests import mini_trainer as T
    world, V = 2, 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_dp_train_worker, args=(r, world, port, q, V, exchange)) for r in range(world)]
    for p in procs:
        p.start()
    case, opt = _dp_case_and_opt()
    nthreads = torch.get_num_threads()
    torch.set_num_threads(2)
    try:
        ref = T.train(case, opt, "oracle", eval_every=60, seed=0, views_per_step=world * V, return_model=True, views_per_rank=V,
                      exchange=exchange)
    finally:
        torch.set_num_threads(nthreads)
    ref_sig = _model_signature(ref["model"])
    res = sorted(q.get(timeout=800) for _ in range(world))
    for p in procs:
        p.join(30)
    assert [r[1] for r in res] == ["ok", "ok"], res
    assert res[0][2] == res[1][2], "the two ranks hold different models"
    assert len(set(ref["P"])) >= 2, ref["P"]
    assert res[0][3] == ref["P"] and res[0][2] == ref_sig, (res[0][3], ref["P"])
    assert res[0][4] == ref["psnr"]
