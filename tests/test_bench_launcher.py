"""bench.py --gpus N must START N ranks (round-1 verdict: the flag used to be parsed and ignored).

CPU: the launcher, the rendezvous, the code-length exchange and the JSON contract with IREC_BENCH_LAUNCH_ONLY=1 (gloo,
no GPU work).  GPU box (one MI355X): the real bench with two ranks sharing the device over gloo."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _run(args, env_extra, timeout=600):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(env_extra)
    return subprocess.run([sys.executable, BENCH] + args, env=env, capture_output=True, text=True, timeout=timeout)


@pytest.mark.parametrize("n", [1, 2, 3])
def test_launcher_starts_n_ranks_cpu_rig(n):
    r = _run(["--gpus", str(n), "--steps", "2", "--warmup", "1"], {"IREC_BENCH_LAUNCH_ONLY": "1"}, timeout=180)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1                                    # ONE JSON line, from rank 0
    res = json.loads(lines[0])
    assert res["n_gpus"] == n and res["world_size"] == n and res["ranks_timed"] == n
    assert res["steps"] == 2 and res["warmup"] == 1


def test_driver_command_rehearsal_eight_ranks():
    """The driver's own N = 8 command line, rehearsed on the CPU (gloo, launch-only: rendezvous, sharding exchange, max-over-ranks
    timing and the JSON contract -- no GPU work): `python -m torch.distributed.run --nnodes=1 --nproc-per-node 8 --master-addr
    127.0.0.1 --master-port P bench.py --gpus 8 --steps K --warmup W`.  One JSON line from rank 0 with n_gpus = world_size = 8,
    eight per-rank entries, weak scaling, and neither the secondary configurations nor the CPU baselines (they run at N = 1 only)."""
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update({"IREC_BENCH_LAUNCH_ONLY": "1", "OMP_NUM_THREADS": "1"})
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "8", "--master-addr", "127.0.0.1",
           "--master-port", str(port), BENCH, "--gpus", "8", "--steps", "3", "--warmup", "2"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    res = json.loads(lines[0])
    assert res["n_gpus"] == 8 and res["world_size"] == 8 and res["ranks_timed"] == 8
    assert len(res["per_rank_latents_per_s"]) == 8 and all(v > 0 for v in res["per_rank_latents_per_s"])
    assert res["scaling"] == "weak" and res["steps"] == 3 and res["warmup"] == 2 and res["higher_is_better"] is True
    assert "cpu_baseline" not in res and "cpu_baseline_opt" not in res and "secondary" not in res
    assert res["metric"] == "encoded latents/sec" and res["unit"] == "latents/s" and res["value"] is None   # never a measurement
    # the launcher form of the same job (`python bench.py --gpus 8`: the parent starts the ranks itself)
    r2 = _run(["--gpus", "8", "--steps", "1", "--warmup", "1"], {"IREC_BENCH_LAUNCH_ONLY": "1", "OMP_NUM_THREADS": "1"}, timeout=600)
    assert r2.returncode == 0, r2.stderr[-2000:]
    res2 = json.loads([ln for ln in r2.stdout.splitlines() if ln.startswith("{")][-1])
    assert res2["n_gpus"] == 8 and res2["world_size"] == 8 and len(res2["per_rank_latents_per_s"]) == 8


def test_world_size_mismatch_is_an_error():
    r = _run(["--gpus", "2"], {"IREC_BENCH_LAUNCH_ONLY": "1", "WORLD_SIZE": "3", "RANK": "0"}, timeout=60)
    assert r.returncode != 0 and "WORLD_SIZE" in (r.stderr + r.stdout)


def test_a_failing_rank_fails_the_job():
    # without the launch-only switch and without a GPU every rank exits non-zero ("no CPU fallback"): the launcher must
    # report failure instead of relaying a line
    import torch
    if torch.cuda.is_available():
        pytest.skip("needs a box without a GPU")
    r = _run(["--gpus", "2", "--steps", "1", "--warmup", "1", "--no-cpu-baseline"], {}, timeout=180)
    assert r.returncode != 0 and not [ln for ln in r.stdout.splitlines() if ln.startswith("{")]


@pytest.mark.gpu
def test_two_ranks_on_one_gpu_over_gloo():
    r = _run(["--gpus", "2", "--steps", "2", "--warmup", "1", "--latents", "4096", "--full", "--no-cpu-baseline"],
             {"IREC_DIST_BACKEND": "gloo"}, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert res["n_gpus"] == 2 and res["world_size"] == 2 and res["backend"] == "gloo"
    assert len(res["per_rank_latents_per_s"]) == 2 and res["value"] > 0
    assert res["roofline"]["kernel"].startswith("encode_") and res["scaling"] == "weak"


@pytest.mark.gpu
def test_single_rank_line_is_self_describing():
    r = _run(["--steps", "2", "--warmup", "1", "--latents", "256", "--full", "--no-cpu-baseline"], {}, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert res["n_gpus"] == 1 and res["roofline"]["kernel"] == "encode_team_kernel<20,3,1>"
    assert res["roofline"]["bound"] == "hbm" and 0 < res["roofline"]["frac"] < 1
    assert res["secondary"]["lds_hw"]["peak"] == 32.0 and res["secondary"]["n_cu"] == 256
    # round 6: the object the driver keeps says what binds the kernel, and carries the other configurations compactly
    b = res["roofline"]["binding"]
    assert b["pipe"] == "lds_gather" and b["hw_peak"] == 32.0 and b["microbench_peak"] == 13.68
    assert {"achieved", "frac_hw", "frac_microbench", "lds_conflict_frac", "lds_busy", "valu_busy"} <= set(b)
    assert abs(b["frac_hw"] - b["achieved"] / 32.0) < 1e-12 and 0 < b["frac_microbench"] < 1.2
    # ... and what the card drew over the timed region against its cap (amdgpu hwmon; None where the files are missing)
    assert {"power_w", "power_cap_w"} <= set(b) and (b["power_w"] is None or 100 < b["power_w"] < 2000)
    cfg = res["roofline"]["configs"]
    assert len(cfg) == 8 and all({"name", "kernel", "ms_per_call", "lookups_per_clk_per_cu"} <= set(c) for c in cfg)
    assert any("configs[3] settings" in c["name"] and c["kernel"].startswith("encode_ten_kernel") for c in cfg)
    assert sum("configs[4]" in c["name"] for c in cfg) == 2 and any("342 blocks" in c["name"] for c in cfg)


@pytest.mark.gpu
def test_rccl_code_path_with_a_world_of_one():
    """The collectives of the N-rank job (process group on RCCL, barrier, all_gather_into_tensor of the code lengths,
    all_gather of the rank times) executed for real over the nccl backend with one rank -- all a 1-GPU box can run."""
    r = _run(["--steps", "2", "--warmup", "1", "--latents", "128", "--full", "--no-cpu-baseline"],
             {"IREC_BENCH_FORCE_DIST": "1", "IREC_DIST_BACKEND": "nccl"}, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert res["n_gpus"] == 1 and res["world_size"] == 1 and res["backend"] == "nccl" and res["value"] > 0


def test_options_of_a_plain_and_a_full_run():
    r = _run(["--help"], {}, timeout=60)
    assert r.returncode == 0 and "--full" in r.stdout and "--dump-outputs" in r.stdout


@pytest.mark.gpu
def test_plain_run_dumps_the_outputs_of_its_last_step(tmp_path):
    """A plain run: the headline only (no decoder leg, secondary configurations or CPU baselines), --steps timed steps, and
    --dump-outputs writes what the timed path returned -- the same files from two runs of the same arguments, and what the
    oracle computes for the dumped latents (1100 latents: the indices and samples of a seeded 1024 of them)."""
    import numpy as np
    import torch
    import bench
    from oracle import oracle as O
    L, lines = 1100, []
    for run in ("a", "b"):
        r = _run(["--steps", "3", "--warmup", "1", "--latents", str(L), "--dump-outputs", str(tmp_path / run)], {}, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        lines.append(json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]))
    res = lines[0]
    assert res["metric"] == "encoded latents/sec" and res["unit"] == "latents/s" and res["higher_is_better"] is True
    assert res["dtype"] == "f32" and res["steps"] == 3 and res["warmup"] == 1 and res["full"] is False
    assert res["value"] > 0 and abs(res["ms_per_step"] - 1e3 * L / res["value"]) < 1e-6 * res["ms_per_step"]
    assert "cpu_baseline" not in res and "decode_ms" not in res["secondary"] and res["roofline"]["configs"] == []
    names = {"K", "code_nats", "latent_ids", "indices", "sample"}
    assert {f.name for f in (tmp_path / "a").iterdir()} == {n + ".npy" for n in names}
    a = {n: np.load(tmp_path / "a" / (n + ".npy")) for n in names}
    b = {n: np.load(tmp_path / "b" / (n + ".npy")) for n in names}
    assert all(a[n].dtype in (np.float32, np.float64) and np.array_equal(a[n], b[n]) for n in names)
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    ids = a["latent_ids"].astype(np.int64)
    assert len(ids) == 1024 and len(np.unique(ids)) == 1024 and ids.max() < L
    assert a["K"].shape == (L, 9) and a["code_nats"].shape == (L,) and a["indices"].shape == (1024, 9, 32)
    assert a["sample"].shape == (1024, bench.N_DIMS)
    # the dumped latents against the oracle, on the inputs the run drew (the bench's seeded generator on this device)
    q = bench.synthetic_batch(L, torch.device("cuda", 0), 0)
    pick = ids[[0, 1, 1023]]
    hb = [t[torch.from_numpy(pick).cuda()].cpu().numpy() for t in q]
    S = int(np.exp(bench.OMEGA * bench.EPS1))
    ridx, rsamp, _ = O.encode_tensors_omp(*hb, bench.SEED, bench.OMEGA, S, bench.BEAMS, bench.BLOCK_SIZE, max_K=32, n_threads=4)
    for n, i in enumerate(pick):
        row = int(np.searchsorted(ids, i))
        for j in range(9):
            k = int(a["K"][i, j])
            assert a["indices"][row, j, :k].astype(np.int64).tolist() == ridx[n][j] and (a["indices"][row, j, k:] == -1).all()
        assert np.array_equal(a["sample"][row], rsamp[n].reshape(-1))
    assert np.allclose(a["code_nats"][pick], a["K"][pick].sum(axis=1) * np.log(S))
