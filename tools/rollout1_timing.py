"""Collect time of the one-hidden-layer policy's rollouts: the graph-replayed step loop
(use_graph=True, the default path) against the one-launch rollout (one_launch_mlp1=True), at
FrozenLake-v1:ppo and Taxi-v3:ppo's preset shapes and one wide shape.

  python tools/rollout1_timing.py --json profiles/rollout1_timing.json
  python tools/rollout1_timing.py --arms graph --package-dir <other checkout>/gymnasium-solver_amd
        the baseline arm alone on a build of another commit (it calls only interfaces that commit
        has), to confirm the default path has not moved

Each collector.collect() is timed by HIP events on the launch stream.  Both arms live in one
process and alternate rollout by rollout after `--warmup` rollouts per arm (the step graph is
captured on the second); reported per arm: the median of `--rollouts` rollouts, min / max and the
quartiles, in ms, with the source hash of the kernels (gsamd.buildinfo).  A second pass times the
T vector steps alone the same way (`steps_only`: the graph replay or the launch, without the value
bootstrap, GAE and episode statistics that both arms share)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHAPES = (("FrozenLake-v1", "ppo", {}),                                   # 32 x 2048
          ("Taxi-v3", "ppo", {}),                                         # 32 x 1024
          ("FrozenLake-v1", "ppo", {"n_envs": 4096, "n_steps": 32}))      # wide
ARMS = {"graph": dict(use_graph=True), "one_launch": dict(use_graph=True, one_launch_mlp1=True)}


def _timed(run, torch):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    run()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def _steps_only(name, coll):
    """The arm's T vector steps alone, as collect() runs them (mode 0): the graph replay or the one
    launch, without the value bootstrap, GAE and episode statistics both arms share."""
    if name == "graph":
        return lambda: coll._collect_steps_graph(0)
    return lambda: coll._collect_one_launch(0)


def _summary(ms):
    q = statistics.quantiles(ms, n=4)
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
            "q1_ms": round(q[0], 4), "q3_ms": round(q[2], 4), "rollouts": len(ms)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rollouts", type=int, default=20, help="timed rollouts per arm (at least 20)")
    ap.add_argument("--warmup", type=int, default=3, help="untimed rollouts per arm first (at least 2: the capture)")
    ap.add_argument("--arms", nargs="+", default=list(ARMS), choices=list(ARMS))
    ap.add_argument("--package-dir", default=os.path.join(ROOT, "gymnasium-solver_amd"),
                    help="the directory that holds the gsamd package and its built library")
    ap.add_argument("--json", default=None, help="write the record here")
    a = ap.parse_args()
    if a.rollouts < 20 or a.warmup < 2:
        ap.error("--rollouts must be at least 20 and --warmup at least 2")
    sys.path[:0] = [os.path.abspath(a.package_dir)]

    import torch
    from gsamd import buildinfo
    from gsamd._lib import lib
    from gsamd.config import load_config
    from gsamd.ppo_agent import DevicePPOAgent

    # the hash build_lib.py embedded into the loaded library; beside it the sources on disk, when
    # the package directory has them (a bare copy of another commit's build does not)
    source_hash = (lib.gs_build_source_hash(b"") or b"").decode()
    if os.path.isdir(buildinfo.CSRC) and buildinfo.source_hash() != source_hash:
        raise SystemExit(f"the library was built from other sources ({source_hash}) than {buildinfo.CSRC}")
    out = {"unit": "ms per collect() (rollout + last value + GAE + episode window), HIP events",
           "arms": {"graph": "captured step loop (gs_policy_act + gs_tabular_step per vector step), one replay",
                    "one_launch": "gs_rollout1_tabular, one launch per rollout"},
           "arms_run": a.arms, "warmup_rollouts": a.warmup, "source_hash": source_hash,
           "device": torch.cuda.get_device_name(0), "results": []}
    for env_id, variant, over in SHAPES:
        colls = {}
        for name in a.arms:
            torch.manual_seed(42)
            agent = DevicePPOAgent(load_config(env_id, variant, overrides=over), device=torch.device("cuda:0"),
                                   track_stats=False, **ARMS[name])
            coll = agent.get_rollout_collector("train")
            if bool(getattr(coll, "one_launch_mlp1", False)) != (name == "one_launch") or coll.one_launch:
                raise SystemExit(f"{name}: the collector did not take that path for {env_id}:{variant} {over}")
            for _ in range(a.warmup):
                coll.collect()
            colls[name] = (agent, coll)
        torch.cuda.synchronize()
        if "graph" in colls and colls["graph"][1]._graphs.get(0) is None:
            raise SystemExit("graph: the step graph was not captured during the warm-up")
        ms, steps = {name: [] for name in colls}, {name: [] for name in colls}
        for _ in range(a.rollouts):
            for name, (_, coll) in colls.items():
                ms[name].append(_timed(coll.collect, torch))
        for _ in range(a.rollouts):
            for name, (_, coll) in colls.items():
                steps[name].append(_timed(_steps_only(name, coll), torch))
        cfg = next(iter(colls.values()))[0].config
        row = {"env": f"{env_id}:{variant}", "n_envs": cfg.n_envs, "n_steps": cfg.n_steps,
               **{name: dict(_summary(v), steps_only=_summary(steps[name])) for name, v in ms.items()}}
        if len(ms) == 2:
            row["graph_over_one_launch"] = round(row["graph"]["median_ms"] / row["one_launch"]["median_ms"], 3)
            row["graph_over_one_launch_steps_only"] = round(
                row["graph"]["steps_only"]["median_ms"] / row["one_launch"]["steps_only"]["median_ms"], 3)
        out["results"].append(row)
        print(json.dumps(row), flush=True)
        del colls
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
