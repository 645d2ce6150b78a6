"""CPU: bench.py's own rank launcher (`python bench.py --gpus N` with no external launcher)
gives every child the torch.distributed.run environment, forwards rank 0's JSON line, and
stops the job when one rank fails (gloo stand-in for the GPU ranks)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE = os.path.join(ROOT, "tests", "_launch_probe.py")

_DRIVER = """
import sys
sys.path.insert(0, {root!r})
import bench
sys.exit(bench.launch_ranks({n}, {argv!r}, script={probe!r}))
"""


def _run(n, argv, timeout=180):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    code = _DRIVER.format(root=ROOT, n=n, argv=list(argv), probe=PROBE)
    return subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=timeout, env=env)


def test_rank_environments():
    import bench
    envs = bench.rank_environments(4, {"X": "1"}, 29511)
    assert [e["RANK"] for e in envs] == ["0", "1", "2", "3"]
    assert [e["LOCAL_RANK"] for e in envs] == ["0", "1", "2", "3"]
    assert all(e["WORLD_SIZE"] == "4" and e["MASTER_ADDR"] == "127.0.0.1" and e["MASTER_PORT"] == "29511"
               and e["X"] == "1" for e in envs)


@pytest.mark.parametrize("n", [2, 4])
def test_launcher_runs_n_ranks(n):
    r = _run(n, ["--gpus", str(n), "--steps", "3"])
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [json.loads(x) for x in r.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1, r.stdout        # only rank 0's line on stdout
    ln = lines[0]
    assert ln["rank"] == 0 and ln["world"] == n and ln["gpus"] == n and ln["steps"] == 3
    assert ln["sum"] == n * (n + 1) / 2     # every rank joined the same group
    assert ln["master"].startswith("127.0.0.1:")
    others = [json.loads(x) for x in r.stderr.splitlines() if x.startswith("{")]
    assert sorted(o["local_rank"] for o in others) == list(range(1, n))


def test_launcher_propagates_a_rank_failure():
    r = _run(2, ["--gpus", "2", "--fail-rank", "1"], timeout=120)
    assert r.returncode == 3, (r.returncode, r.stderr[-2000:])


def test_dump_outputs_writes_float32_arrays_and_a_fixed_sample(tmp_path, monkeypatch):
    """--dump-outputs: every array of the last step as float32 .npy; one above the element cap is
    written as the same seeded sample of its elements on every run."""
    from types import SimpleNamespace as NS
    import numpy as np
    import torch
    import bench
    monkeypatch.setattr(bench, "DUMP_MAX_ELEMS", 64)
    T, N = 4, 8
    g = torch.Generator().manual_seed(0)
    f = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    buf = NS(obs=(torch.rand(T, N, 5, generator=g) * 255).to(torch.uint8), actions=torch.arange(T * N).reshape(T, N),
             logprobs=f(T, N), values=f(T, N), rewards=f(T, N), dones=torch.zeros(T, N, dtype=torch.uint8),
             advantages=f(T, N), returns=f(T, N), last_values=f(N))
    agent = NS(policy_model=NS(params=f(40)), adam_m=f(40), adam_v=f(40), metrics_buf=f(3, 7),
               get_rollout_collector=lambda stage: NS(buffer=buf))
    bench.dump_outputs(agent, str(tmp_path / "a"))
    bench.dump_outputs(agent, str(tmp_path / "b"))
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(os.listdir(tmp_path / "b")) and len(names) == 13
    for n in names:
        a, b = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert a.dtype == np.float32 and a.size <= 64 and np.array_equal(a, b), n
    assert np.array_equal(np.load(tmp_path / "a" / "params.npy"), agent.policy_model.params.numpy())
    assert np.array_equal(np.load(tmp_path / "a" / "rollout_actions.npy"), buf.actions.numpy().astype(np.float32))
    obs = np.load(tmp_path / "a" / "rollout_obs.npy")          # 160 elements > 64: sampled
    assert obs.shape == (64,) and set(obs.tolist()) <= set(buf.obs.reshape(-1).tolist())


def test_bench_has_full_and_dump_outputs_options():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0 and "--full" in r.stdout and "--dump-outputs" in r.stdout


def test_bench_rejects_mismatched_world():
    env = dict(os.environ, WORLD_SIZE="2", RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "4"], capture_output=True,
                       text=True, timeout=120, env=env)
    assert r.returncode != 0 and "must agree" in r.stderr
