"""Multi-process pair sharding (cs566-project-lightglue_amd/parallel.py) on CPU with gloo, world
size 2.  The per-rank matcher is the CPU oracle (test stand-in for the HIP model): the test checks
the sharding / gather plumbing, so the sharded result must equal one unsharded run exactly."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _setup(prune=False):
    import lgamd  # noqa: F401
    import oracle
    from lightglue_amd.weights import synthetic_pair, synthetic_state_dict

    conf = {"filter_threshold": 0.1, "n_layers": 2}
    if prune:  # per-pair cost varies: width pruning + early stop (configs[3]'s regime)
        conf.update(width_confidence=0.9, depth_confidence=0.9)
    sd = synthetic_state_dict(conf, seed=0)
    if prune:
        sd["log_assignment.0.matchability.bias"][:] = -2.0  # prunes part of the points at layer 0
    B = 7 if prune else 5
    data = {k: torch.from_numpy(v) for k, v in synthetic_pair(B=B, M=40, N=36, seed=2).items()}

    def matcher(d):
        # the oracle follows the reference's B == 1 pruning (lightglue.py:528,533): one pair at a
        # time, stacked (the HIP forward batches the chunk instead)
        outs = [oracle.lightglue_forward(sd, {k: v[i : i + 1].numpy() for k, v in d.items()}, conf)
                for i in range(d["keypoints0"].shape[0])]
        return {k: torch.cat([o[k] for o in outs]) for k in ("matches0", "matches1", "matching_scores0", "matching_scores1")}

    return matcher, data


def _worker(rank, world, port, mode, out_dir):
    import sys

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import lgamd  # noqa: F401
        from lightglue_amd import parallel

        torch.set_num_threads(1)
        matcher, data = _setup(prune=mode.endswith("prune"))
        if mode == "static":
            res = parallel.match_static(matcher, data)
        else:
            chunk = 1 if mode == "dynamic" else 3
            # two calls in a row: every call gets its own queue counter (no reset between calls)
            for _ in range(2):
                res, done = parallel.match_dynamic(matcher, data, chunk=chunk)
            torch.save(torch.tensor(done, dtype=torch.int64).reshape(-1, 2), os.path.join(out_dir, f"done{rank}.pt"))
        torch.save(res, os.path.join(out_dir, f"res{rank}.pt"))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("mode", ["static", "dynamic", "dynamic_chunked", "dynamic_chunked_prune"])
def test_sharded_matches_equal_unsharded(tmp_path, mode):
    import sys

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    world = 2
    mp.spawn(_worker, args=(world, _free_port(), mode, str(tmp_path)), nprocs=world, join=True)
    matcher, data = _setup(prune=mode.endswith("prune"))
    # the unsharded run on one thread like the workers: torch's CPU products sum in an order that
    # depends on the thread count, and the comparison below is exact
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        ref = matcher(data)
    finally:
        torch.set_num_threads(threads)
    for r in range(world):
        res = torch.load(tmp_path / f"res{r}.pt", weights_only=True)
        for k in ("matches0", "matches1", "matching_scores0", "matching_scores1"):
            np.testing.assert_array_equal(res[k].numpy(), ref[k].numpy(), err_msg=f"rank {r} {k}")
    if mode.startswith("dynamic"):
        chunks = sum((torch.load(tmp_path / f"done{r}.pt", weights_only=True).tolist() for r in range(world)), [])
        pairs = sorted(i for a, b in chunks for i in range(a, b))
        assert pairs == list(range(data["keypoints0"].shape[0]))  # every pair exactly once
        if mode != "dynamic":
            assert max(b - a for a, b in chunks) > 1  # pairs really travel in chunks


def test_guided_chunks_shrink_towards_the_tail():
    import lgamd  # noqa: F401
    from lightglue_amd.parallel import guided_chunk

    assert guided_chunk(512, 8, 32) == 32
    assert guided_chunk(100, 8, 32) == 13
    assert guided_chunk(3, 8, 32) == 1
    assert guided_chunk(3, 8, 32, min_chunk=2) == 2
    # single process: the whole queue in chunks of at most `chunk`
    seen, rem, sizes = 0, 70, []
    while seen < rem:
        c = guided_chunk(rem - seen, 1, 32)
        sizes.append(min(c, rem - seen))
        seen += c
    assert sizes == [32, 32, 6]


def test_match_dynamic_without_process_group():
    """World size 1 (no process group): the same chunk loop on a local counter."""
    import lgamd  # noqa: F401
    from lightglue_amd import parallel

    matcher, data = _setup()
    res, done = parallel.match_dynamic(matcher, data, chunk=2)
    assert done == [(0, 2), (2, 4), (4, 5)]
    ref = matcher(data)
    for k in ("matches0", "matches1", "matching_scores0", "matching_scores1"):
        np.testing.assert_array_equal(res[k].numpy(), ref[k].numpy())


def test_shard_range_covers_batch():
    import lgamd  # noqa: F401
    from lightglue_amd.parallel import shard_range

    for B in range(0, 20):
        for world in (1, 2, 3, 8):
            idx = []
            for r in range(world):
                a, b = shard_range(B, world, r)
                idx += list(range(a, b))
            assert idx == list(range(B))


def _bench_json(cmd, env=None):
    import json
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    e = dict(os.environ, OMP_NUM_THREADS="1")
    e.pop("WORLD_SIZE", None)
    e.update(env or {})
    r = subprocess.run([sys.executable] + cmd, cwd=root, env=e, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_bench_spawns_gpus_ranks_itself():
    """bench.py --gpus 2 without a launcher spawns two ranks (CPU/gloo rehearsal): n_gpus and the
    pair count cover both ranks, and the step goes through parallel.match_static."""
    res = _bench_json(["bench.py", "--gpus", "2", "--selftest-cpu", "--steps", "3", "--warmup", "1",
                       "--batch", "3", "--npts", "32", "--cpu-budget", "0"])
    assert res["n_gpus"] == 2
    assert res["pairs_timed"] == 3 * 3 * 2
    assert res["config"]["global_batch"] == 6
    assert "match_static" in res["config"]["parallelism"]
    assert res["value"] == pytest.approx(res["pairs_timed"] / (res["ms_per_step"] * res["steps"] / 1000.0), rel=1e-2)


@pytest.mark.parametrize("full", [False, True])
def test_bench_plain_run_is_lean_and_full_adds_the_rest(tmp_path, full):
    """A plain run times --steps steps, reports ms_per_step and writes --dump-outputs; the CPU
    baseline appears only with --full (CPU rehearsal with the stand-in matcher)."""
    out = tmp_path / "dump"
    res = _bench_json(["bench.py", "--gpus", "1", "--selftest-cpu", "--steps", "4", "--warmup", "1", "--batch", "2",
                       "--npts", "16", "--cpu-budget", "0.05", "--dump-outputs", str(out)] + (["--full"] if full else []))
    assert res["steps"] == 4 and res["pairs_timed"] == 4 * 2
    assert res["ms_per_step"] >= 0 and res["value"] > 0  # the stand-in's steps take microseconds
    assert ("cpu_baseline" in res) == full
    assert sorted(os.listdir(out)) == ["matches0.npy", "matches1.npy", "matching_scores0.npy", "matching_scores1.npy"]
    m0 = np.load(out / "matches0.npy")
    assert m0.dtype == np.float64 and m0.shape == (2, 16) and (m0 == -1).all()
    assert np.load(out / "matching_scores0.npy").dtype == np.float32


def test_bench_under_torchrun_launcher():
    port = _free_port()
    res = _bench_json(["-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                       "--master-port", str(port), "bench.py", "--gpus", "2", "--selftest-cpu", "--steps", "2",
                       "--warmup", "1", "--batch", "2", "--npts", "16", "--cpu-budget", "0"])
    assert res["n_gpus"] == 2 and res["pairs_timed"] == 2 * 2 * 2


def test_bench_rejects_world_size_mismatch():
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, WORLD_SIZE="2", RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--selftest-cpu", "--cpu-budget", "0"], cwd=root,
                       env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "WORLD_SIZE=2" in (r.stderr + r.stdout)


@pytest.mark.parametrize("workload,path", [("configs3", "match_dynamic"), ("configs4", "match_static")])
def test_bench_workload_rehearsals(workload, path):
    """bench.py --workload configs3 / configs4 through two spawned gloo ranks (CPU stand-in
    matcher): configs3 pulls guided chunks from the shared queue, configs4 runs static shards."""
    res = _bench_json(["bench.py", "--gpus", "2", "--selftest-cpu", "--steps", "2", "--warmup", "1",
                       "--batch", "5", "--npts", "16", "--cpu-budget", "0", "--workload", workload, "--chunk", "2"])
    assert res["n_gpus"] == 2 and res["pairs_timed"] == 2 * 5 * 2
    assert path in res["config"]["parallelism"]
    assert res["config"]["workload"].startswith(workload)


def test_exchange_bytes_within_twice_the_result_size():
    """at configs[3] (64 pairs per GPU x 8 ranks, N = 2048) the bytes one
    match_dynamic call moves through the collective stay within 2x the packed result size, under
    guided chunks and even with an unlucky split of the queue (one rank taking an extra chunk)."""
    import lgamd  # noqa: F401
    from lightglue_amd.parallel import exchange_bytes, guided_chunk

    B, N, world = 512, 2048, 8
    result = B * (4 + 8 * (N + N))  # one packed int32 row per pair
    # simulate the shared queue with the ranks pulling round-robin
    counts, seen, r = [0] * world, 0, 0
    while seen < B:
        c = min(guided_chunk(B - seen, world, 32), B - seen)
        counts[r % world] += c
        seen += c
        r += 1
    assert sum(counts) == B
    assert exchange_bytes(B, N, N, world, counts) <= 2 * result
    skew = list(counts)
    skew[0] += 32
    skew[1] -= 32
    assert exchange_bytes(B, N, N, world, skew) <= 2 * result
    # the round-3 exchange: an all_reduce of the whole B x (2M + 2N) float64 buffer
    assert exchange_bytes(B, N, N, world, counts) < B * (4 * N) * 8
    assert exchange_bytes(B, N, N, world) <= 1.01 * result  # static shards


@pytest.mark.parametrize("workload", ["train", "train_sg"])
def test_bench_training_rehearsal_two_ranks(workload):
    """bench.py --workload train / train_sg through two spawned gloo ranks: the
    CPU stand-in is the float32 oracle training step with the data-parallel semantics of
    ddp.DataParallel (gradients averaged over the ranks, SuperGlue's BatchNorms synchronised)."""
    res = _bench_json(["bench.py", "--gpus", "2", "--selftest-cpu", "--steps", "1", "--warmup", "1", "--batch", "1",
                       "--npts", "16", "--cpu-budget", "0", "--workload", workload])
    assert res["n_gpus"] == 2 and res["config"]["global_batch"] == 2
    assert "data-parallel x2" in res["config"]["parallelism"]
    assert ("SyncBatchNorm" in res["config"]["parallelism"]) == (workload == "train_sg")
    assert np.isfinite(res["loss"]) and res["value"] > 0
