"""Workload for the rollout (collect) evidence: one workload's device rollouts only (no update),
for `rocprofv3 --kernel-trace --stats`.

  python tools/collect_run.py [C5|C4|C3|C2] [rollouts]          a bench workload (synthetic env)
  python tools/collect_run.py --env Acrobot-v1 [--variant ppo] [--n-envs N] [--one-launch {0,1}]
                                                                  a config's own device env
  python tools/collect_run.py --env Acrobot-v1 --n-envs 32 1024 --ab --json out.json
        A/B of the one-launch rollout against the graph-replayed step loop of the same build: both
        arms in one process, alternated, `--warmup` rollouts per arm first (the graph is captured
        on the second), then `--repeats` timed blocks of `rollouts` rollouts per arm.

  python tools/collect_run.py --env MountainCar-v0 --variant ppo_curiosity --override model_id=mlp_small \
        --override env_wrappers=[] ...
        `--override K=V` (repeatable) sets a config field after resolution, as train.py's option
        does; V is read as JSON where it parses (numbers, lists, null), else as a string.

Prints the mean collect time per rollout from HIP events on the launch stream."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "gymnasium-solver_amd")]

import torch  # noqa: E402

from gsamd.config import load_config  # noqa: E402
from gsamd.ppo_agent import DevicePPOAgent  # noqa: E402


def _collector(env_id, variant, over, one_launch):
    torch.manual_seed(42)
    cfg = load_config(env_id, variant, overrides=over)
    agent = DevicePPOAgent(cfg, device=torch.device("cuda:0"), track_stats=False,
                           **({} if one_launch is None else {"one_launch": bool(one_launch)}))
    return agent, agent.get_rollout_collector("train"), cfg


def _timed(coll, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        coll.collect()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / n


def _ab(a, env_id, over):
    out = {"env": f"{env_id}:{a.variant}", "overrides": {k: v for k, v in over.items() if k != "n_envs"},
           "rollouts_per_block": a.rollouts, "warmup_rollouts": a.warmup,
           "arms": {"one_launch": "gs_rollout_env, one launch per rollout",
                    "graph": "captured step loop (gs_policy_act + env step per vector step), one replay per rollout"},
           "unit": "ms per rollout (collect: rollout + last value + GAE + episode window), HIP events", "results": []}
    for n_envs in a.n_envs:
        arms = {}
        for name, one in (("one_launch", 1), ("graph", 0)):
            agent, coll, cfg = _collector(env_id, a.variant, dict(over, n_envs=n_envs), one)
            if coll.one_launch != bool(one):
                raise SystemExit(f"{name}: the collector did not take that path at n_envs={n_envs}")
            for _ in range(a.warmup):
                coll.collect()
            arms[name] = (agent, coll)
        torch.cuda.synchronize()
        blocks = {name: [] for name in arms}
        for _ in range(a.repeats):
            for name, (_, coll) in arms.items():
                blocks[name].append(round(_timed(coll, a.rollouts), 4))
        row = {"n_envs": n_envs, "n_steps": cfg.n_steps, "blocks_ms": blocks,
               "mean_ms": {k: round(sum(v) / len(v), 4) for k, v in blocks.items()},
               "spread_ms": {k: round(max(v) - min(v), 4) for k, v in blocks.items()}}
        row["graph_over_one_launch"] = round(row["mean_ms"]["graph"] / row["mean_ms"]["one_launch"], 3)
        out["results"].append(row)
        print(json.dumps(row), flush=True)
        del arms
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("workload", nargs="?", default=None, help="bench workload (C2..C5); default C5 without --env")
    ap.add_argument("rollouts", nargs="?", type=int, default=None, help="timed rollouts (default 3; --ab: 20)")
    ap.add_argument("--env", default=None, help="env id of a config with device dynamics (instead of a workload)")
    ap.add_argument("--variant", default="ppo")
    ap.add_argument("--n-envs", type=int, nargs="+", default=None, help="override n_envs (--ab: one or more)")
    ap.add_argument("--one-launch", type=int, choices=(0, 1), default=None,
                    help="1: the one-launch rollout where supported (the default), 0: the step loop / graph")
    ap.add_argument("--ab", action="store_true", help="alternate one-launch and graph arms in this process")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--json", default=None, help="--ab: write the record here")
    ap.add_argument("--override", action="append", default=[], metavar="K=V",
                    help="set config field K to V after resolution (V as JSON where it parses); repeatable")
    a = ap.parse_args()
    if a.workload is not None and a.workload.isdigit() and a.rollouts is None:      # --env ... [rollouts]
        a.workload, a.rollouts = None, int(a.workload)
    if a.env:
        env_id, over, tag = a.env, {}, f"{a.env}:{a.variant}"
    else:
        import bench      # only the bench workloads need its table
        tag = a.workload or "C5"
        env_id, a.variant, n_envs = bench.WORKLOADS[tag]
        over = dict(n_envs=n_envs, env_dynamics="synthetic")
    for kv in a.override:
        k, sep, v = kv.partition("=")
        if not sep:
            ap.error(f"--override takes K=V, got {kv!r}")
        try:
            over[k] = json.loads(v)
        except ValueError:
            over[k] = v
    if a.ab:
        a.rollouts = a.rollouts or 20
        if not a.n_envs:
            a.n_envs = [int(over.get("n_envs") or load_config(env_id, a.variant).n_envs)]
        return _ab(a, env_id, over)
    if a.n_envs:
        over["n_envs"] = a.n_envs[0]
    n = a.rollouts or 3
    agent, coll, cfg = _collector(env_id, a.variant, over, a.one_launch)
    for _ in range(max(1, a.warmup - 1)):
        coll.collect()
    torch.cuda.synchronize()
    ms = _timed(coll, n)
    path = "one launch" if coll.one_launch else ("step graph" if coll.use_graph else "step loop")
    print(f"{tag}: {cfg.n_envs} envs x {cfg.n_steps} steps ({path}): collect {ms:.3f} ms per rollout "
          f"({ms * 1e3 / cfg.n_steps:.1f} us per vector step)")


if __name__ == "__main__":
    main()
