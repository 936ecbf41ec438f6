"""bench.py's process plumbing, without a GPU: `--gpus N` must start N ranks itself (before any GPU call), and a
torchrun environment whose WORLD_SIZE disagrees with --gpus must be refused.  The processes that must see no GPU get every device
hidden (HIP_VISIBLE_DEVICES=-1: device ids end at the first invalid one), so these checks hold on a host with GPUs as well."""
import json
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO_GPU = {"HIP_VISIBLE_DEVICES": "-1", "CUDA_VISIBLE_DEVICES": "-1"}


def _run(args, env_extra=None, timeout=300):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    env.update(env_extra or {})
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=env, capture_output=True, text=True,
                          timeout=timeout, cwd=ROOT)


def test_gpus_n_refuses_a_node_with_fewer_gpus():
    """No GPU visible: --gpus 2 must fail loudly (not run one rank and print n_gpus: 1)."""
    r = _run(["--gpus", "2"], NO_GPU)
    assert r.returncode != 0
    assert "shows 0 GPU" in r.stderr


def test_gpus_n_starts_n_ranks_before_any_gpu_call():
    """With the one-device rehearsal switch the parent launches torch.distributed.run with 2 ranks; with every GPU hidden
    each rank announces itself and then stops at 'needs an MI355X' — which proves rank processes were started with
    WORLD_SIZE=2 and that the parent itself never needed a GPU to get there (torchrun ends the sibling of the first rank
    to fail, so one announcement is enough)."""
    r = _run(["--gpus", "2", "--workload", "cfg2"], {"NCF_BENCH_SINGLE_DEVICE": "1", "NCF_BENCH_BACKEND": "gloo", "NCF_BENCH_ANNOUNCE": "1", **NO_GPU})
    assert r.returncode != 0
    assert " of 2 (local rank" in r.stderr and "bench.py needs an MI355X" in r.stderr, r.stderr[-2000:]


def test_world_size_must_match_gpus():
    r = _run(["--gpus", "4"], {"WORLD_SIZE": "2", "RANK": "0", "LOCAL_RANK": "0"})
    assert r.returncode != 0
    assert "--gpus 4 but WORLD_SIZE=2" in r.stderr


def test_steps_must_be_positive():
    r = _run(["--steps", "0"])
    assert r.returncode != 0
    assert "--steps must be >= 1" in r.stderr


def test_dump_outputs_is_refused_for_a_secondary_workload(tmp_path):
    r = _run(["--workload", "cfg3", "--dump-outputs", str(tmp_path / "out")])
    assert r.returncode != 0
    assert "--dump-outputs writes the headline workload's outputs" in r.stderr
    assert not (tmp_path / "out").exists()


def test_secondary_workload_needs_full():
    r = _run(["--workload", "cfg3"], NO_GPU)
    assert r.returncode != 0
    assert "--workload cfg3 is a secondary config: it runs with --full only" in r.stderr


@pytest.mark.gpu
def test_plain_run_measures_the_headline_alone(gpu):
    """A plain run prints the headline line without what --full adds, and spends less than 30 s outside its steps."""
    import time
    steps, warmup = 20, 5
    t0 = time.perf_counter()
    r = _run(["--gpus", "1", "--steps", str(steps), "--warmup", str(warmup)], timeout=600)
    wall = time.perf_counter() - t0
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads([s for s in r.stdout.splitlines() if s.startswith("{")][-1])
    assert line["metric"] == "scored user-item pairs/sec" and line["unit"] == "pairs/s" and line["dtype"] == "f32"
    assert line["higher_is_better"] is True and line["steps"] == steps and line["value"] > 0 and line["ms_per_step"] > 0
    assert line["config"]["full"] is False
    for key in ("roofline", "gather_roofline", "variants", "cpu_baseline", "cpu_baseline_reference_formulation", "other_configs"):
        assert key not in line
    assert wall - (steps + warmup) * line["ms_per_step"] * 1e-3 < 30.0


@pytest.mark.gpu
def test_dump_outputs_holds_the_last_timed_step(gpu, tmp_path):
    """--dump-outputs DIR: the scores of the last of the --steps timed steps (40 steps over the 16 cycled index batches: the
    last one scores batch 39 % 16), equal to the same seeded model on the same batch computed here."""
    import numpy as np
    sys.path.insert(0, ROOT)
    import bench
    steps = 40
    r = _run(["--workload", "cfg2", "--steps", str(steps), "--warmup", "1", "--no-cpu-baseline", "--no-variants",
              "--dump-outputs", str(tmp_path / "out")], timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads([s for s in r.stdout.splitlines() if s.startswith("{")][-1])
    assert line["steps"] == steps
    got = np.load(tmp_path / "out" / "scores.npy")
    assert got.dtype == np.float32 and got.shape == (bench.B, 1)
    model = bench.make_model(gpu)
    iu, ii = bench.make_batches(gpu, 0)[(steps - 1) % bench.N_BATCHES]
    with torch.no_grad():
        want = model(iu, ii).cpu().numpy()
    assert np.array_equal(got, want)
