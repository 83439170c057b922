"""bench.py starts its own ranks: `python bench.py --gpus N` with no launcher in the environment must come back with ONE rank-0 JSON
line that reports N.  CPU: the launch plumbing over gloo (--dry-run: rendezvous + one all-reduce, no GPU
work); the full N-rank run over RCCL is tests/test_parallel_gpu.py (needs >= 2 GPUs)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, env_extra=None, timeout=240):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    if "--dry-run" in args:  # the launch plumbing over gloo on any host (RCCL would bind one GPU per rank: none on a CPU host, one on a 1-GPU box)
        env["TAD_DIST_BACKEND"] = "gloo"
    env.update(env_extra or {})
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True, timeout=timeout, env=env)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    return r, lines


@pytest.mark.timeout(300)
def test_bench_self_launches_n_ranks_and_prints_one_line():
    r, lines = _run(["--gpus", "2", "--dry-run"])
    assert r.returncode == 0, r.stderr[-2000:]
    assert len(lines) == 1, r.stdout
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["allreduce_of_ones"] == 2.0 and out["launched_by"] == "self"


@pytest.mark.timeout(120)
def test_bench_single_rank_needs_no_launcher():
    r, lines = _run(["--gpus", "1", "--dry-run"])
    assert r.returncode == 0 and len(lines) == 1 and json.loads(lines[0])["n_gpus"] == 1


@pytest.mark.timeout(300)
def test_bench_scaling_flags_reach_every_rank():
    """the flags of the first multi-GPU run (tools/scale_run.sh): strong scaling splits --global-batch over the ranks, --linear-schedule and
    --bucket-dtype are accepted and echoed by the launch plumbing"""
    r, lines = _run(["--gpus", "2", "--dry-run", "--global-batch", "256", "--linear-schedule", "persistent", "--bucket-dtype", "bf16"])
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(lines[0])
    assert out["flags"] == {"linear_schedule": "persistent", "bucket_dtype": "bf16", "global_batch": 256, "per_gpu_batch": 128, "scaling": "strong"}
    r, lines = _run(["--gpus", "2", "--dry-run"])
    assert json.loads(lines[0])["flags"] == {"linear_schedule": "auto", "bucket_dtype": "f32", "global_batch": 0, "per_gpu_batch": 32, "scaling": "weak"}
    r, _ = _run(["--gpus", "1", "--dry-run", "--bucket-dtype", "fp8"])
    assert r.returncode != 0


def test_rccl_summary_reads_the_debug_lines(tmp_path):
    """`collective.rccl` quotes RCCL's own description of the communicator: parsed from NCCL_DEBUG=INFO text (format of RCCL 2.2x)"""
    sys.path.insert(0, ROOT)
    import bench
    log = tmp_path / "rccl.log"
    log.write_text("\n".join([
        "host:1:1 [0] NCCL INFO RCCL version 2.26.6+hip7.0 HEAD:abc",
        "host:1:1 [0] NCCL INFO comm 0x1 rank 0 nranks 8 cudaDev 0 busId 1000 - Init START",
        "host:1:1 [0] NCCL INFO Channel 00/0 : 0[0] -> 1[1] via P2P/IPC",
        "host:1:1 [0] NCCL INFO Channel 01/0 : 0[0] -> 7[7] via P2P/IPC",
        "host:1:1 [0] NCCL INFO Channel 01/0 : 3[3] -> 4[4] via P2P/IPC",
        "host:1:1 [0] NCCL INFO 16 coll channels, 16 nvls channels, 16 p2p channels, 2 p2p channels per peer"]))
    s = bench.rccl_summary(str(log))
    assert s["channels"] == 2 and s["transports"] == ["P2P/IPC"] and s["peers_of_rank0"] == [1, 7]
    assert s["transport_of_rank0"] == "xGMI peer-to-peer" and any("RCCL version" in ln for ln in s["lines"])
    assert "not collected" in bench.rccl_summary(None)["debug_lines"]


def test_power_sampler_reads_hwmon_and_picks_the_loaded_card(tmp_path):
    """bench.py's `power` object: board power / cap / shader clock from the amdgpu hwmon files, the card under load = the one with the highest
    mean power (the container sees every card of the host), joules per step = mean power x step time; no card readable -> an error entry, not
    an exception"""
    import time
    sys.path.insert(0, ROOT)
    import bench
    for i, (uw, cap, hz) in enumerate(((250_000_000, 1_400_000_000, 97_000_000), (1_395_000_000, 1_400_000_000, 2_135_000_000))):
        d = tmp_path / f"class/drm/card{i}/device/hwmon/hwmon{i}"
        d.mkdir(parents=True)
        (d / "power1_average").write_text(str(uw))
        (d / "power1_cap").write_text(str(cap))
        (d / "freq1_input").write_text(str(hz))
    ps = bench.PowerSampler(period=0.01, sysfs_root=str(tmp_path)).start()
    time.sleep(0.08)
    per = ps.stop()
    assert len(per) == 2 and per[0]["mean_w"] == 250.0 and per[1]["mean_w"] == 1395.0 and per[1]["n"] >= 3
    out = ps.summary(per, seconds_per_step=0.0422)
    assert out["mean_w"] == 1395.0 and out["cap_w"] == 1400.0 and out["frac_of_cap"] == 0.9964 and out["mean_sclk_mhz"] == 2135
    assert out["joules_per_step"] == round(1395.0 * 0.0422, 2) and "index 1" in out["source"]
    empty = bench.PowerSampler(sysfs_root=str(tmp_path / "nothing")).start()
    assert "error" in empty.summary(empty.stop())
    share = bench.host_cpu_share()
    assert share["os_cpu_count"] >= share["usable"] >= 1


def test_bench_steps_must_be_positive():
    """`--steps` is the number of timed steps: zero of them cannot give `ms_per_step` (refused before anything is imported or launched)"""
    for bad in (["--steps", "0"], ["--warmup", "-1"]):
        r, lines = _run(["--gpus", "1"] + bad, timeout=60)
        assert r.returncode == 2 and not lines and "--steps must be >= 1" in r.stderr


def test_dump_outputs_writes_float32_arrays_and_a_fixed_parameter_sample(tmp_path):
    """--dump-outputs: every array as float32 .npy, a scalar as shape (1,), small parameter tensors in full and large ones at the same
    seeded positions in every run (so that two builds can be compared element for element)"""
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import bench
    torch.manual_seed(0)
    m = torch.nn.Sequential(torch.nn.Linear(100, 64), torch.nn.Linear(64, 3))  # 6400-element weight: sampled; the rest in full
    outs = {"loss": torch.tensor(0.5, dtype=torch.float64), "logits": torch.randn(4, 3, dtype=torch.bfloat16), "grad_norm": torch.tensor(2.0)}
    shapes = bench.dump_outputs(str(tmp_path / "a"), outs, m, per_tensor=4096)
    assert shapes == {"loss": [1], "logits": [4, 3], "grad_norm": [1], "params_sample": [4096 + 64 + 192 + 3]}
    got = {k: np.load(tmp_path / "a" / (k + ".npy")) for k in shapes}
    assert all(a.dtype == np.float32 for a in got.values())
    assert got["loss"][0] == 0.5 and np.array_equal(got["logits"], outs["logits"].float().numpy())
    p = got["params_sample"]
    w0 = m[0].weight.detach().reshape(-1).numpy()
    assert np.isin(p[:4096], w0).all() and np.array_equal(p[4096:], np.concatenate([m[0].bias.detach().numpy(), m[1].weight.detach().reshape(-1).numpy(),
                                                                                       m[1].bias.detach().numpy()]))
    bench.dump_outputs(str(tmp_path / "b"), {}, m, per_tensor=4096)
    assert np.array_equal(np.load(tmp_path / "b" / "params_sample.npy"), p)


@pytest.mark.gpu
@pytest.mark.timeout(600)
def test_plain_bench_run_times_its_steps_and_dumps_the_last_one(tmp_path):
    """`bench.py --gpus 1` without --full: the headline fields and nothing measured beside them; --dump-outputs holds the last timed step's
    loss (the line's `loss`), logits, gradient norm and updated parameters"""
    import numpy as np
    r, lines = _run(["--gpus", "1", "--steps", "2", "--warmup", "1", "--batch", "2", "--dump-outputs", str(tmp_path / "out")], timeout=540)
    assert r.returncode == 0 and len(lines) == 1, (r.returncode, r.stderr[-3000:])
    out = json.loads(lines[0])
    assert out["steps"] == 2 and out["warmup"] == 1 and out["ms_per_step"] > 0 and out["value"] > 0 and out["higher_is_better"] is True
    assert out["unit"] == "clips/sec" and out["dtype"] == "bf16" and out["metric"].startswith("clips/sec")
    assert not {"roofline", "power", "from_profiles", "roofline_all", "half", "precise", "cpu_baseline"} & set(out)
    arrays = {k: np.load(tmp_path / "out" / (k + ".npy")) for k in ("loss", "logits", "grad_norm", "params_sample")}
    assert out["dump_outputs"]["arrays"] == {k: list(a.shape) for k, a in arrays.items()}
    assert arrays["logits"].shape == (2, 2) and all(a.dtype == np.float32 and np.isfinite(a).all() for a in arrays.values())
    assert abs(float(arrays["loss"][0]) - out["loss"]) <= 1e-6 * max(1.0, abs(out["loss"]))
