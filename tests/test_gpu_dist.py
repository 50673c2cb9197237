"""Multi-process path on REAL kernels without a multi-GPU node: two ranks share the one GPU of the box (gloo carries the
collectives; on the 8-GPU node the same code runs one rank per GPU over RCCL).  Each rank renders its ray shard and its shard of the
collocation points with the HIP path, gradients land in the GradBucket / PdeGradStage exactly as in bench.py, and after the split
all-reduce the averaged gradient must equal the single-process gradient of the union batch."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import GOLD, ROOT
from helpers import make_model, named_grads

pytestmark = pytest.mark.gpu
T = 19.0 / 60.0
W_PDE = 0.7


def _local_grads(model, o, d, u, tgt, pts, tt, bucket, stage, world, streams=False):
    """bench.Step's gradient path for one rank's shard: in-place accumulation into the bucket, PDE term through the stage.
    streams=True is the order of bench.Step._step_streams with several ranks: PDE chain and render on their own HIP streams, the head
    all-reduce started as soon as the render is differentiated, commit + tail all-reduce after the PDE chain has joined."""
    f = model.nvfi
    f.train()
    f.accumulate_grads_inplace = True
    bucket.zero()
    tail = bucket.tail_offset(list(f.vel.parameters()))
    model.vel_loss_weight = W_PDE
    model.vel_grad_targets = stage.views

    def render_term():
        f.jitter_override = u
        try:
            out = f(T, o, d, True)
        finally:
            f.jitter_override = None
        torch.nn.functional.mse_loss(out[0], tgt).backward()

    if not streams:
        render_term()
        h = bucket.all_reduce_head_start(tail)
        stage.zero()
        model.get_vel_loss(points=pts, t=tt)
        stage.commit_device(f.last_pde_out)
        bucket.all_reduce_finish(h, tail)
        return
    main = torch.cuda.current_stream()
    s_pde, s_r = torch.cuda.Stream(), torch.cuda.Stream()
    start = torch.cuda.Event(); start.record(main)
    with torch.cuda.stream(s_pde):
        s_pde.wait_event(start)
        stage.zero()
        model.get_vel_loss(points=pts, t=tt)
        pde_out = f.last_pde_out
    with torch.cuda.stream(s_r):
        s_r.wait_event(start)
        render_term()
    main.wait_stream(s_r)
    h = bucket.all_reduce_head_start(tail)
    main.wait_stream(s_pde)
    stage.commit_device(pde_out)
    bucket.all_reduce_finish(h, tail)


def _worker(rank, world, port, out, streams, backend="gloo", exchange="torch"):
    """backend "gloo": both ranks on device 0 (the 1-GPU box); "nccl": one rank per GPU over RCCL (needs >= 2 devices).
    exchange "abi": the gradient sum goes through nvfi_allreduce_grads (RcclComm) instead of torch.distributed.all_reduce."""
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), HSA_ENABLE_IPC_MODE_LEGACY="0")
    sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
    dev = rank if backend == "nccl" else 0
    torch.cuda.set_device(dev)
    if backend == "nccl":
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", dev))
    else:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    from nvfi_amd.dist import GradBucket, PdeGradStage, shard_range
    if exchange == "abi":
        return _worker_abi(rank, world, out)
    gold = np.load(os.path.join(GOLD, "hotpath.npz"))
    model, meta = make_model("A")
    f = model.nvfi
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    R, P = gold["A:rays_o"].shape[0], gold["A:pde:points"].shape[0]
    lo, hi = shard_range(R, rank, world)
    plo, phi = shard_range(P, rank, world)
    params = [p for g in model.get_optparam_groups() for p in g["params"]]
    bucket = GradBucket(params)
    stage = PdeGradStage(f._pde_params())
    _local_grads(model, cu(gold["A:rays_o"][lo:hi]), cu(gold["A:rays_d"][lo:hi]), torch.from_numpy(gold["A:train_nonkey:u"][lo:hi].copy()),
                 cu(gold["A:train_nonkey:target"][lo:hi]), cu(gold["A:pde:points"][plo:phi]), cu(gold["A:pde:t"][plo:phi]), bucket, stage, world, streams)
    torch.cuda.synchronize()
    if rank == 0:
        g = named_grads(model)
        np.savez(out, **{k: v for k, v in g.items() if v is not None}, n_kept=float(f.last_pde_out[1]))
    dist.barrier()
    dist.destroy_process_group()


def _worker_abi(rank, world, out):
    """NVFI_ALLREDUCE=abi order of bench.Step: render + PDE term accumulate locally (PDE through the stage, weighted on the device by
    W*n_r/sum n_r), then ONE nvfi_allreduce_grads(average) of the flat buffer over the RcclComm."""
    from nvfi_amd.dist import GradBucket, PdeGradStage, RcclComm, shard_range
    gold = np.load(os.path.join(GOLD, "hotpath.npz"))
    model, meta = make_model("A", f"cuda:{torch.cuda.current_device()}")
    f = model.nvfi
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    R, P = gold["A:rays_o"].shape[0], gold["A:pde:points"].shape[0]
    lo, hi = shard_range(R, rank, world)
    plo, phi = shard_range(P, rank, world)
    bucket = GradBucket([p for g in model.get_optparam_groups() for p in g["params"]])
    stage = PdeGradStage(f._pde_params())
    comm = RcclComm()
    assert comm.world == world and comm.rank == rank
    f.train(); f.accumulate_grads_inplace = True
    bucket.zero(); stage.zero()
    model.vel_loss_weight = W_PDE
    model.vel_grad_targets = stage.views
    f.jitter_override = torch.from_numpy(gold["A:train_nonkey:u"][lo:hi].copy())
    o = f(T, cu(gold["A:rays_o"][lo:hi]), cu(gold["A:rays_d"][lo:hi]), True)
    f.jitter_override = None
    torch.nn.functional.mse_loss(o[0], cu(gold["A:train_nonkey:target"][lo:hi])).backward()
    model.get_vel_loss(points=cu(gold["A:pde:points"][plo:phi]), t=cu(gold["A:pde:t"][plo:phi]))
    stage.commit_device(f.last_pde_out)
    bucket.all_reduce_mean(comm)
    torch.cuda.synchronize()
    if rank == 0:
        g = named_grads(model)
        np.savez(out, **{k: v for k, v in g.items() if v is not None}, n_kept=float(f.last_pde_out[1]))
    dist.barrier()
    comm.close()
    dist.destroy_process_group()


def _union_batch_reference():
    """single process, union batch (same kernels, plain autograd accumulation)"""
    gold = np.load(os.path.join(GOLD, "hotpath.npz"))
    model, meta = make_model("A")
    f = model.nvfi
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    f.train()
    f.jitter_override = torch.from_numpy(gold["A:train_nonkey:u"].copy())
    try:
        o = f(T, cu(gold["A:rays_o"]), cu(gold["A:rays_d"]), True)
    finally:
        f.jitter_override = None
    loss = torch.nn.functional.mse_loss(o[0], cu(gold["A:train_nonkey:target"]))
    lv = model.get_vel_loss(points=cu(gold["A:pde:points"]), t=cu(gold["A:pde:t"]))
    (loss + W_PDE * lv).backward()
    return named_grads(model), int(f.last_pde_n_kept)


def _assert_matches_union(got):
    ref, n_kept = _union_batch_reference()
    n = 0
    for k, r in ref.items():
        if r is None or k == "basis_mat_density.weight":
            continue
        err = np.abs(got[k] - r).max() / (np.abs(r).max() + 1e-30)
        assert err < 5e-4, (k, err)        # fp32 sums in a different order (shard-wise, atomics)
        n += 1
    assert n >= 40, n
    assert 0 < float(got["n_kept"]) < n_kept      # rank 0 kept only its share of the points


needs_two_gpus = pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs >= 2 GPUs (one RCCL rank per device); enables itself on a multi-GPU node")


@needs_two_gpus
@pytest.mark.parametrize("exchange,streams", [("torch", False), ("torch", True), ("abi", False)])
def test_two_rccl_ranks_match_the_union_batch(tmp_path, exchange, streams):
    """One rank per GPU over RCCL ("nccl"): the split torch.distributed all-reduce (with and without the three-stream order) and the
    C-ABI exchange nvfi_allreduce_grads (NVFI_ALLREDUCE=abi in bench.py) all reproduce the single-process gradient of the union batch."""
    out = str(tmp_path / "g2.npz")
    port = 29900 + (os.getpid() % 1500) + (3 if streams else 0) + (5 if exchange == "abi" else 0)
    mp.spawn(_worker, args=(2, port, out, streams, "nccl", exchange), nprocs=2, join=True)
    _assert_matches_union(np.load(out))


def _run_bench(extra, env=None, timeout=900):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py")] + extra
    return subprocess.run(cmd, env=dict(os.environ, **(env or {})), capture_output=True, text=True, timeout=timeout)


def test_bench_gpus_flag_starts_the_ranks_itself():
    """`python bench.py --gpus 2` (no launcher in front): on a node with >= 2 GPUs it starts 2 RCCL ranks and reports n_gpus 2 from the
    process group; on the 1-GPU box it must refuse loudly (non-zero exit, a message that says why) instead of running one process."""
    r = _run_bench(["--gpus", "2", "--steps", "2", "--warmup", "1", "--grid", "64", "--pts", "16384", "--prime", "1", "--no-cpu-baseline"])
    if torch.cuda.device_count() >= 2:
        assert r.returncode == 0, r.stderr[-2000:]
        d = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
        assert d["n_gpus"] == 2 and d["process_group"]["ranks"] == 2 and len(d["process_group"]["devices"]) == 2
        assert d["process_group"]["backend"].startswith("nccl") and d["value"] > 0
    else:
        assert r.returncode != 0
        assert "needs 2 GPUs" in r.stderr and not [ln for ln in r.stdout.splitlines() if ln.startswith("{")]


def test_bench_gpus_flag_spawns_gloo_ranks_on_one_gpu():
    """Same self-spawn path, exercised end to end on the 1-GPU box: NVFI_BENCH_BACKEND=gloo lets the two ranks share the device."""
    r = _run_bench(["--gpus", "2", "--steps", "2", "--warmup", "1", "--grid", "64", "--pts", "16384", "--prime", "1", "--no-cpu-baseline"],
                   env=dict(NVFI_BENCH_BACKEND="gloo"))
    assert r.returncode == 0, r.stderr[-2000:]
    d = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert d["n_gpus"] == 2 and d["process_group"]["ranks"] == 2 and d["process_group"]["backend"] == "gloo"


def test_bench_refuses_a_world_size_that_contradicts_gpus():
    r = _run_bench(["--gpus", "1", "--steps", "1", "--warmup", "0", "--grid", "64", "--no-cpu-baseline"],
                   env=dict(WORLD_SIZE="2", RANK="0", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT="29555"), timeout=300)
    assert r.returncode != 0 and "must agree" in r.stderr


@pytest.mark.parametrize("streams", [False, True])
def test_two_ranks_on_one_gpu_match_the_union_batch(tmp_path, streams):
    out = str(tmp_path / "g2.npz")
    port = 29600 + (os.getpid() % 1500) + (7 if streams else 0)
    mp.spawn(_worker, args=(2, port, out, streams), nprocs=2, join=True)
    got = np.load(out)
    _assert_matches_union(got)


@pytest.mark.parametrize("scaling", ["weak", "strong", "weak-streams"])
def test_bench_runs_as_two_ranks(scaling):
    """bench.py under torch.distributed.run with 2 ranks on the one GPU (NVFI_BENCH_BACKEND=gloo): the multi-rank branch of the step
    (staged PDE gradients, split all-reduce, MAX-over-ranks timing) executes end to end and rank 0 prints one JSON line."""
    env = dict(os.environ, NVFI_BENCH_BACKEND="gloo", MASTER_ADDR="127.0.0.1")
    streams = scaling.endswith("-streams")      # the three-stream step with the split all-reduce under the PDE chain (default with RCCL)
    if streams:
        env["NVFI_OVERLAP"] = "1"
        scaling = "weak"
    port = 29700 + (os.getpid() % 1500) + (1 if scaling == "strong" else 0) + (2 if streams else 0)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", str(port),
           os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--grid", "64", "--pts", "16384", "--prime", "1", "--no-cpu-baseline", "--scaling", scaling,
           "--full"]          # (work_per_step comes from the profiled pass)
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
    d = json.loads(line)
    assert d["n_gpus"] == 2 and d["scaling"] == scaling and d["value"] > 0
    per_gpu = 4096 if scaling == "weak" else 2048
    assert d["config"]["rays_per_step_per_gpu"] == per_gpu
    assert d["work_per_step"]["P_kept"] > 0


def _worker_graph(rank, world, port, out, graphed):
    """bench.Step as one of two gloo ranks on device 0, four iterations on a live field: eager (the three-stream order around the exchange),
    or bench.GraphedStep's multi-rank form - three captured graphs (draw + repack | PDE term | renders + regularisers) replayed around the
    same eager exchange."""
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), HSA_ENABLE_IPC_MODE_LEGACY="0",
                      NVFI_BENCH_BACKEND="gloo", NVFI_OVERLAP="1")
    sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import bench
    dev = torch.device("cuda", 0)
    torch.manual_seed(7); torch.cuda.manual_seed(7)
    model = bench.build_scene(dev, 64, 64, True)
    step = bench.Step(model, dev, 512, 8192, world, rank, "cfg3", live=True)
    step()                                   # optimiser state, workspaces
    torch.manual_seed(11 + rank); torch.cuda.manual_seed(11 + rank)
    step.gen.manual_seed(5 + rank); step.rng = np.random.default_rng(5)      # (frame times: the same on every rank, as in the reference's DDP loop)
    step.seed_override, step.draw_it = 5 + rank, 0
    losses = []
    if graphed:
        gs = bench.GraphedStep(step)
        gs._capture_multi()                  # iteration 1 eagerly through the record, iteration 2 = the first replay of the three graphs
        for _ in range(2):
            gs(); losses.append(float(gs.loss))
        gs.check()
    else:
        for _ in range(4):
            losses.append(float(step()))
    torch.cuda.synchronize()
    if rank == 0:
        np.savez(out, losses=np.asarray(losses[-2:]), **{k: v.detach().cpu().contiguous().numpy() for k, v in model.state_dict().items()
                                                         if v.dtype.is_floating_point and v.numel() > 1})
    dist.barrier()
    dist.destroy_process_group()


def test_captured_two_rank_step_follows_the_eager_one(tmp_path):
    """verdict r4 item 6: the multi-rank step with the host out of the launch chains.  Two gloo ranks on the one GPU; the same seeds and host
    draws -> the last two losses and the parameters after four iterations agree between the eager and the captured form."""
    res = []
    for graphed in (False, True):
        out = str(tmp_path / f"cap{int(graphed)}.npz")
        port = 29900 + (os.getpid() % 1000) + (3 if graphed else 0)
        mp.spawn(_worker_graph, args=(2, port, out, graphed), nprocs=2, join=True)
        res.append(np.load(out))
    e, g = res
    print("eager", e["losses"], "captured", g["losses"])
    np.testing.assert_allclose(g["losses"], e["losses"], rtol=2e-3)
    moved = 0
    for k in e.files:
        if k == "losses":
            continue
        lr = 0.02 if "plane" in k else 1e-3
        assert np.abs(g[k] - e[k]).max() <= 4.1 * lr, k
        assert np.mean(np.abs(g[k] - e[k]) > 2e-2 * 4 * lr) < 0.02, k
        moved += 1
    assert moved >= 19


def test_rccl_abi_allreduce_single_rank():
    """nvfi_allreduce_grads over RCCL behind the C ABI.  A one-rank communicator on the one GPU of the box: unique id, init,
    in-place sum and mean (identity for one rank), on a side stream, then destroy.  (Two ranks cannot share one device in a RCCL
    communicator; N > 1 is the driver's 8-GPU run.)"""
    from nvfi_amd.dist import RcclComm, GradBucket
    comm = RcclComm(world=1, rank=0)
    ps = [torch.nn.Parameter(torch.randn(1, 24, 9, 11, device="cuda").contiguous(memory_format=torch.channels_last)), torch.nn.Parameter(torch.randn(128, 28, device="cuda"))]
    b = GradBucket(ps)
    b.flat.copy_(torch.arange(b.flat.numel(), device="cuda", dtype=torch.float32))
    ref = b.flat.clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        b.all_reduce_mean(comm)
        comm.all_reduce_(b.flat, average=False)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    assert torch.equal(b.flat, ref)
    assert ps[1].grad.data_ptr() == b.flat[ps[0].numel():].data_ptr()
    comm.close()
