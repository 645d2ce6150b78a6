"""Wall time per rollout of the eager step loop on the device CartPole-v1: the path where the
Python cost of DeviceVecEnv.step_into (one gs_cartpole_step call per vector step, beside one
gs_policy_act) is the largest share of a rollout.

  python tools/eager_rollout_timing.py
  python tools/eager_rollout_timing.py --package-dir <other checkout>/gymnasium-solver_amd
        the same measurement on another commit's host code (it calls only interfaces that commit
        has); copy this build's library there when the kernel sources are the same

One process, one DeviceRolloutCollector(use_graph=False, one_launch=False, track_stats=False) on
`--n-envs` x `--n-steps` (32 x 512) with the 64-64 policy of CartPole-v1:ppo; `--warmup` rollouts,
then `--rollouts` timed ones, each from before collect() to after a device synchronize, by
time.perf_counter.  Prints one JSON line: the median, min / max and quartiles in ms, and the
library's source hash."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n-envs", type=int, default=32)
    ap.add_argument("--n-steps", type=int, default=512)
    ap.add_argument("--rollouts", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--package-dir", default=os.path.join(ROOT, "gymnasium-solver_amd"),
                    help="the directory that holds the gsamd package and its built library")
    a = ap.parse_args()
    sys.path[:0] = [os.path.abspath(a.package_dir)]

    import torch
    from gsamd._lib import lib
    from gsamd.policy import DeviceMLPActorCritic
    from gsamd.rollout import DeviceCartPoleVecEnv, DeviceRolloutCollector

    dev = torch.device("cuda:0")
    torch.manual_seed(42)
    env = DeviceCartPoleVecEnv(a.n_envs, seed=42, device=dev)
    pm = DeviceMLPActorCritic(4, (64, 64), 2, device=dev)
    coll = DeviceRolloutCollector(env, pm, a.n_steps, use_graph=False, one_launch=False, track_stats=False)
    if coll.one_launch or coll.one_launch_mlp1 or coll.use_graph:
        raise SystemExit("the collector did not take the eager step loop")
    ms = []
    for i in range(a.warmup + a.rollouts):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        coll.collect()
        torch.cuda.synchronize()
        if i >= a.warmup:
            ms.append((time.perf_counter() - t0) * 1e3)
    q = statistics.quantiles(ms, n=4)
    print(json.dumps({"package_dir": os.path.abspath(a.package_dir), "n_envs": a.n_envs, "n_steps": a.n_steps,
                      "unit": "ms per collect() of the eager step loop, wall clock",
                      "median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3),
                      "max_ms": round(max(ms), 3), "q1_ms": round(q[0], 3), "q3_ms": round(q[2], 3),
                      "rollouts": len(ms), "warmup_rollouts": a.warmup,
                      "source_hash": (lib.gs_build_source_hash(b"") or b"").decode(),
                      "device": torch.cuda.get_device_name(0)}), flush=True)


if __name__ == "__main__":
    main()
