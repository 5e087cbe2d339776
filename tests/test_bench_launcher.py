"""bench.py's rank launcher (VERDICT r5 "missing" #1): ``python bench.py --gpus N`` without a launcher around it starts the N
ranks itself under torch.distributed.run, refuses to run fewer ranks than asked for, and refuses a --gpus that disagrees with
the launcher's WORLD_SIZE.  No GPU needed: these paths end before the first CUDA call."""
import json
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _run(args, **env):
    e = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    e.update(env)
    return subprocess.run([sys.executable, BENCH] + args, env=e, capture_output=True, text=True, timeout=300)


def test_print_launch_is_the_torchrun_line():
    r = _run(["--gpus", "8", "--steps", "20", "--warmup", "5", "--print-launch"])
    assert r.returncode == 0, r.stderr[-2000:]
    argv = json.loads(r.stdout.strip().splitlines()[-1])["launch_argv"]
    assert argv[1:3] == ["-m", "torch.distributed.run"]
    assert "--nnodes=1" in argv and "--nproc-per-node=8" in argv
    assert argv[argv.index("--master-addr") + 1] == "127.0.0.1"
    assert 1024 < int(argv[argv.index("--master-port") + 1]) < 65536
    i = argv.index(BENCH)
    assert argv[i + 1:] == ["--gpus", "8", "--steps", "20", "--warmup", "5"]        # every other argument is handed on


def test_more_ranks_than_gpus_is_an_error_not_a_smaller_run():
    have = torch.cuda.device_count() if torch.cuda.is_available() else 0
    r = _run(["--gpus", str(have + 1)])
    assert r.returncode != 0
    assert f"sees {have} GPU(s)" in r.stderr and f"--gpus {have + 1}" in r.stderr
    assert "{" not in r.stdout, "no JSON line may be printed"


def test_gpus_must_agree_with_the_launchers_world_size():
    r = _run(["--gpus", "2"], WORLD_SIZE="4", RANK="0", LOCAL_RANK="0")
    assert r.returncode != 0 and "WORLD_SIZE = 4" in r.stderr and "{" not in r.stdout


def test_in_process_form_is_one_rank_only():
    r = _run(["--gpus", "2", "--in-process"])
    assert r.returncode != 0 and "ONE rank" in r.stderr


@pytest.mark.gpu
def test_gpus_1_goes_through_the_spawn_path_and_reports_rccl():
    """the driver's single-GPU command: the line must come from a rank started by bench.py's own launcher, on a 1-rank RCCL group
    (--full: a plain run creates no group at N = 1)"""
    r = _run(["--gpus", "1", "--steps", "1", "--warmup", "1", "--full", "--no-cpu-baseline", "--no-extras"])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    la = line["launcher"]
    assert line["n_gpus"] == 1 and la["launched"] and la["spawned_by_bench"] and la["rccl_ranks"] == 1 and la["all_reduce_of_ones"] == 1.0
    assert la["rccl_version"].count(".") == 2
    assert len([ln for ln in r.stdout.splitlines() if ln.strip()]) == 1, "stdout carries exactly ONE line (RCCL's banner goes to stderr)"


@pytest.mark.gpu
def test_a_failing_launcher_does_not_cost_the_single_gpu_line():
    """if the spawned rank dies (here: on purpose) the N = 1 line is measured in the launching process and says so; still ONE line"""
    r = _run(["--gpus", "1", "--steps", "1", "--warmup", "1", "--no-cpu-baseline", "--no-extras"], IPLAN_BENCH_TEST_FAIL_IN_RANK="1")
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    out = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(out) == 1
    la = json.loads(out[0])["launcher"]
    assert la["spawn_failed"] and not la["launched"] and la["rccl_ranks"] is None
    assert "measuring in this process instead" in r.stderr


def test_dump_outputs_writes_the_last_steps_results_emulated(tmp_path):
    """--dump-outputs' writer on a small loop (host-emulated kernels): float32 files of the last rollout's episode and of every net's
    state, the larger ones as a fixed sample, the same values from the same seed"""
    import importlib.util
    import numpy as np
    from iplan_amd import _lib as L
    from iplan_amd.config import default_args
    from iplan_amd.harness import SyntheticLoop
    from tests.emu.emu_lib import get_emu_lib
    spec = importlib.util.spec_from_file_location("bench", BENCH)
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    L.use_library_for_tests(get_emu_lib())
    try:
        outs = []
        for run in range(2):
            args = default_args("highway", use_cuda=False, batch_size_run=2, n_agents=2, max_vehicle_num=7, n_other_vehicles=5,
                                episode_limit=6, max_history_len=3, buffer_size=2, batch_size=1, ppo_epoch=1, pred_batch_size=4,
                                pred_length=2, device="cpu")
            args.obs_shape, args.state_shape = args.obs_shape_single * 5, args.obs_shape_single * args.max_vehicle_num
            np.random.seed(0)
            loop = SyntheticLoop(args, 2, seed=1, device="cpu")
            loop.cycle()
            batch = loop.rollout()
            old, bench.DUMP_SAMPLE = bench.DUMP_SAMPLE, 50
            try:
                info = bench.dump_outputs(loop, batch, str(tmp_path / str(run)))
            finally:
                bench.DUMP_SAMPLE = old
            files = sorted(os.listdir(tmp_path / str(run)))
            assert info["files"] == len(files) == 12 and 0 < info["bytes"] <= bench.DUMP_MAX_BYTES
            arrays = {f: np.load(tmp_path / str(run) / f) for f in files}
            assert all(a.dtype == np.float32 and a.size <= 50 for a in arrays.values())
            assert arrays["episode_actions.npy"].shape == (2, 7, 2, 1) and np.abs(arrays["params_actors.npy"]).sum() > 0
            # the values are the last rollout's fields and the nets' state: whole below the sample size, else at the seeded positions
            assert np.array_equal(arrays["episode_actions.npy"], batch.data["actions"].float().numpy())

            def at_positions(t):
                pos = torch.randperm(t.numel(), generator=torch.Generator().manual_seed(0))[:50].sort().values
                return t.reshape(-1).float()[pos].numpy()
            assert np.array_equal(arrays["episode_attention_latent.npy"], at_positions(batch.data["attention_latent"]))
            actors = torch.cat([v.reshape(-1).float() for m in loop.mac.agents for v in m.state_dict().values() if v.is_floating_point()])
            assert np.array_equal(arrays["params_actors.npy"], at_positions(actors))
            decoder = torch.cat([v.reshape(-1).float() for m in loop.behavior.behavior_decoder for v in m.state_dict().values()
                                 if v.is_floating_point()])
            assert np.array_equal(arrays["params_behavior_decoder.npy"], at_positions(decoder))
            outs.append(arrays)
        for f in outs[0]:
            assert np.array_equal(outs[0][f], outs[1][f]), f
    finally:
        L.use_library_for_tests(None)


@pytest.mark.gpu
def test_plain_line_is_lean_and_dumps_outputs(tmp_path):
    """``--gpus 1 --steps K --warmup W`` without --full: the headline keys, K timed steps, nothing measured beside them; with
    --dump-outputs the float32 files of the last step (64 MB at most)"""
    import numpy as np
    out = tmp_path / "dump"
    r = _run(["--gpus", "1", "--steps", "2", "--warmup", "1", "--dump-outputs", str(out)])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line["steps"] == 2 and line["warmup"] == 1 and line["ms_per_step"] > 0 and line["value"] > 0
    assert line["unit"] == "env-steps/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
    assert abs(line["value"] * line["ms_per_step"] / 1e3 - line["config"]["env_steps_per_step"]) < 1e-6 * line["value"]
    assert not {"roofline", "config5", "config4_n1", "cpu_baseline"} & set(line)
    assert line["launcher"]["spawned_by_bench"] and line["launcher"]["rccl_ranks"] is None
    files = sorted(os.listdir(out))
    assert line["dump_outputs"]["files"] == len(files) and "episode_actions.npy" in files and "params_actors.npy" in files
    arrays = [np.load(out / f) for f in files]
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in arrays)
    assert sum(a.nbytes for a in arrays) <= 64 << 20
