"""bench.py's multi-GPU launch contract, on the CPU (no device here): an N-GPU request either
runs N ranks or fails loudly (VERDICT r02 "Next round" #1)."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _run(args, env_extra=None):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    env.update(env_extra or {})
    return subprocess.run([sys.executable, BENCH] + args, env=env, capture_output=True, text=True, timeout=300)


def test_more_gpus_than_devices_is_refused():
    import torch
    have = torch.cuda.device_count()
    r = _run(["--gpus", str(max(2, have + 1)), "--steps", "1", "--warmup", "0"])
    assert r.returncode == 2, r.stderr
    assert "requested but only" in r.stderr
    assert r.stdout.strip() == ""          # no JSON line for a run that did not happen


def test_world_size_mismatch_is_refused():
    r = _run(["--gpus", "4", "--steps", "1"], {"WORLD_SIZE": "2", "RANK": "0", "LOCAL_RANK": "0"})
    assert r.returncode == 2
    assert "WORLD_SIZE=2 but --gpus 4" in r.stderr


def _bench_module():
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_mod", BENCH)
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    return bench


def test_plain_run_is_the_default(monkeypatch):
    """--full and --dump-outputs are off unless asked for; --steps sets the timed steps and must
    be at least 1 (ms_per_step divides by it)."""
    import pytest
    bench = _bench_module()
    monkeypatch.setattr(sys, "argv", [BENCH, "--gpus", "1", "--steps", "7", "--warmup", "2"])
    args = bench.parse()
    assert (args.full, args.dump_outputs, args.steps, args.warmup) == (False, None, 7, 2)
    monkeypatch.setattr(sys, "argv", [BENCH, "--full", "--dump-outputs", "somewhere"])
    args = bench.parse()
    assert args.full is True and args.dump_outputs == "somewhere"
    monkeypatch.setattr(sys, "argv", [BENCH, "--steps", "0"])
    with pytest.raises(SystemExit):
        bench.parse()


def test_launcher_builds_a_torchrun_child(monkeypatch):
    """launch_ranks hands torchrun N ranks on 127.0.0.1 and this script, and returns its status."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_mod", BENCH)
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    seen = {}

    def fake_call(cmd):
        seen["cmd"] = cmd
        return 7

    import subprocess as sp
    monkeypatch.setattr(sp, "call", fake_call)
    monkeypatch.setattr(sys, "argv", [BENCH, "--gpus", "2", "--rehearse-one-gpu", "--steps", "3"])
    args = bench.parse()
    assert bench.launch_ranks(args) == 7
    cmd = seen["cmd"]
    assert cmd[1:4] == ["-m", "torch.distributed.run", "--nnodes=1"]
    assert cmd[cmd.index("--nproc-per-node") + 1] == "2"
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1"
    assert cmd[-5:] == [os.path.abspath(BENCH), "--gpus", "2", "--rehearse-one-gpu", "--steps", "3"][-5:]
