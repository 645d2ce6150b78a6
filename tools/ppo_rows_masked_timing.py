"""Step time of the masked row-parallel PPO update (gs_ppo_rows_update_masked, valid [0, 3, 4] of 18
actions) beside the unmasked entry (gs_ppo_rows_update) on the same rollout, at the two Pong-objects
shapes (12-128-128-18, 12-64-18) and B = 2048 and 8192.

  python tools/ppo_rows_masked_timing.py --json profiles/ppo_rows_masked_timing.json

The method is tools/ppo_rows_timing.py's: a window is one call of `--steps` optimizer steps
(minibatches drawn with replacement from a random rollout whose recorded actions are valid ones), timed
by HIP events on the launch stream; both arms live in one process and alternate window by window
after `--warmup` windows per arm; reported per arm: the `--repeats` step times in us, their median and
their spread (max - min).

Gate, at every shape: the masked arm's median step time is no larger than the unmasked arm's plus the
spread of the unmasked arm's repeats (the masked row forms the exponentials of the valid actions only)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

VALID = (0, 3, 4)
CASES = (((12, 128, 128, 18), 2048), ((12, 128, 128, 18), 8192), ((12, 64, 0, 18), 2048), ((12, 64, 0, 18), 8192))
ARMS = ("unmasked", "masked")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=300, help="optimizer steps per window (at least 200)")
    ap.add_argument("--warmup", type=int, default=2, help="untimed windows per arm first (at least 2)")
    ap.add_argument("--repeats", type=int, default=5, help="timed windows per arm (at least 3)")
    ap.add_argument("--package-dir", default=os.path.join(ROOT, "gymnasium-solver_amd"),
                    help="the directory that holds the gsamd package and its built library")
    ap.add_argument("--json", default=None, help="write the record here")
    a = ap.parse_args()
    if a.steps < 200 or a.warmup < 2 or a.repeats < 3:
        ap.error("--steps must be at least 200, --warmup at least 2 and --repeats at least 3")
    sys.path[:0] = [os.path.abspath(a.package_dir)]

    import torch
    from gsamd import buildinfo
    from gsamd._lib import MlpDims, PPOHparams, RolloutView, check, lib

    source_hash = (lib.gs_build_source_hash(b"") or b"").decode()
    if os.path.isdir(buildinfo.CSRC) and buildinfo.source_hash() != source_hash:
        raise SystemExit(f"the library was built from other sources ({source_hash}) than {buildinfo.CSRC}")
    dev = torch.device("cuda:0")
    n = a.steps
    mask = sum(1 << v for v in VALID)
    out = {"unit": "us per optimizer step (one call of `steps` minibatches / steps), HIP events",
           "arms": {"unmasked": "gs_ppo_rows_update (GS_HP_ACT_STATS on, normalize_adv on: the agent's defaults)",
                    "masked": f"gs_ppo_rows_update_masked, valid {list(VALID)} (the same flags, rollout and indices)"},
           "steps": n, "warmup_windows": a.warmup, "repeats": a.repeats, "source_hash": source_hash,
           "device": torch.cuda.get_device_name(0), "results": []}
    hp = PPOHparams(0.2, 0.2, 0.5, 0.01, 0.5, 3e-4, 0.9, 0.999, 1e-8, 0.0, 1, 2)
    for dims, B in CASES:
        D = dims[0]
        d = MlpDims(*dims)
        P = int(lib.gs_mlp_param_count(d))
        g = torch.Generator(device="cpu").manual_seed(1234 + B + D)
        T, N = 8, max(2048, B)
        roll = dict(obs=torch.randn(T, N, D, generator=g),
                    actions=torch.tensor(VALID)[torch.randint(0, len(VALID), (T, N), generator=g)],
                    logprobs=-torch.rand(T, N, generator=g) - 0.2, values=torch.randn(T, N, generator=g),
                    advantages=torch.randn(T, N, generator=g), returns=torch.randn(T, N, generator=g))
        roll = {k: v.to(dev).contiguous() for k, v in roll.items()}
        view = RolloutView(*(roll[k].data_ptr() for k in ("obs", "actions", "logprobs", "values", "advantages", "returns")),
                           T, N)
        idx = torch.randint(0, T * N, (n * B,), generator=g, dtype=torch.int32).to(dev)
        p0 = (0.05 * torch.randn(P, generator=g)).to(dev)
        nbytes = int(lib.gs_ppo_rows_workspace_bytes(d, B))
        if nbytes == 0:
            raise SystemExit(f"{dims} at B = {B} is not served")
        z = lambda: torch.zeros(P, device=dev)  # noqa: E731
        state = {arm: dict(p=p0.clone(), g=z(), m=z(), v=z(), ws=torch.zeros(nbytes, dtype=torch.uint8, device=dev),
                           met=torch.zeros(n, 40, device=dev), stop=torch.zeros(1, dtype=torch.int32, device=dev), step=0)
                 for arm in ARMS}

        def window(arm):
            s = state[arm]
            args = (s["p"].data_ptr(), s["g"].data_ptr(), s["m"].data_ptr(), s["v"].data_ptr(), d, hp, view, idx.data_ptr(),
                    B, n, s["step"], s["met"].data_ptr(), s["stop"].data_ptr(), s["ws"].data_ptr(), s["ws"].numel(), None,
                    torch.cuda.current_stream().cuda_stream)
            check(lib.gs_ppo_rows_update_masked(*args, mask) if arm == "masked" else lib.gs_ppo_rows_update(*args), arm)
            s["step"] += n

        def timed(arm):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            window(arm)
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1) * 1000.0 / n

        for _ in range(a.warmup):
            for arm in ARMS:
                window(arm)
        torch.cuda.synchronize()
        us = {arm: [] for arm in ARMS}
        for _ in range(a.repeats):
            for arm in ARMS:
                us[arm].append(timed(arm))
        row = {"dims": list(dims), "batch": B, "valid": list(VALID)}
        for arm in ARMS:
            if not torch.isfinite(state[arm]["met"]).all() or not torch.isfinite(state[arm]["p"]).all():
                raise SystemExit(f"{arm}: non-finite records or parameters at {dims}, B = {B}")
            med = statistics.median(us[arm])
            row[arm] = {"step_us": [round(x, 3) for x in us[arm]], "median_us": round(med, 3),
                        "spread_us": round(max(us[arm]) - min(us[arm]), 3), "rows_per_s": round(B / med * 1e6)}
        row["gate_masked_le_unmasked_plus_unmasked_spread"] = bool(
            row["masked"]["median_us"] <= row["unmasked"]["median_us"] + row["unmasked"]["spread_us"])
        out["results"].append(row)
        print(json.dumps(row), flush=True)
        del state, roll
    out["gate"] = all(r["gate_masked_le_unmasked_plus_unmasked_spread"] for r in out["results"])
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    print("gate:", out["gate"])


if __name__ == "__main__":
    main()
