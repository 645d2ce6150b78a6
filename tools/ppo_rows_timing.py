"""Step time of the row-parallel PPO update (gs_ppo_rows_update) beside the REINFORCE update
(gs_pg_update, the same data flow on the vector ALUs without the value head) and, for context, the
chain (gs_ppo_update) at its own batch size.

  python tools/ppo_rows_timing.py --json profiles/ppo_rows_timing.json

A window is one call of `--steps` optimizer steps (minibatches drawn with replacement from a random
rollout), timed by HIP events on the launch stream; the step time is the window's time / steps.
All arms of a shape live in one process and alternate window by window after `--warmup` windows per
arm; reported per arm: the `--repeats` step times in us, their median and their spread (max - min).

Gate: at the two shapes both updates serve, (10, 128, 128, 10) and (4, 256, 256, 2) at B = 2048, the
rows update's median step time is no larger than gs_pg_update's plus the spread of gs_pg_update's
repeats.  The other rows (Pong-objects dims at B = 2048 and 8192, two and one hidden layers; the chain
at B = 256) are context: rows per second."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (dims (D, H1, H2, A), batch, arms)
CASES = (((10, 128, 128, 10), 2048, ("rows", "pg")),
         ((4, 256, 256, 2), 2048, ("rows", "pg")),
         ((12, 128, 128, 18), 2048, ("rows",)),
         ((12, 128, 128, 18), 8192, ("rows",)),
         ((12, 64, 0, 18), 2048, ("rows",)),
         ((12, 64, 0, 18), 8192, ("rows",)),
         ((4, 256, 256, 2), 256, ("chain",)))
GATED = {((10, 128, 128, 10), 2048), ((4, 256, 256, 2), 2048)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=300, help="optimizer steps per window (at least 200)")
    ap.add_argument("--warmup", type=int, default=2, help="untimed windows per arm first (at least 1)")
    ap.add_argument("--repeats", type=int, default=3, help="timed windows per arm (at least 3)")
    ap.add_argument("--package-dir", default=os.path.join(ROOT, "gymnasium-solver_amd"),
                    help="the directory that holds the gsamd package and its built library")
    ap.add_argument("--json", default=None, help="write the record here")
    a = ap.parse_args()
    if a.steps < 200 or a.warmup < 1 or a.repeats < 3:
        ap.error("--steps must be at least 200, --warmup at least 1 and --repeats at least 3")
    sys.path[:0] = [os.path.abspath(a.package_dir)]

    import torch
    from gsamd import buildinfo
    from gsamd._lib import MlpDims, PGHparams, PPOHparams, RolloutView, check, lib

    source_hash = (lib.gs_build_source_hash(b"") or b"").decode()
    if os.path.isdir(buildinfo.CSRC) and buildinfo.source_hash() != source_hash:
        raise SystemExit(f"the library was built from other sources ({source_hash}) than {buildinfo.CSRC}")
    dev = torch.device("cuda:0")
    n = a.steps
    out = {"unit": "us per optimizer step (one call of `steps` minibatches / steps), HIP events",
           "arms": {"rows": "gs_ppo_rows_update (GS_HP_ACT_STATS on, normalize_adv on: the agent's defaults)",
                    "pg": "gs_pg_update (normalize_targets on)",
                    "chain": "gs_ppo_update, captured graph (the agent's default), GS_HP_ACT_STATS on"},
           "steps": n, "warmup_windows": a.warmup, "repeats": a.repeats, "source_hash": source_hash,
           "device": torch.cuda.get_device_name(0), "results": []}
    ppo_hp = PPOHparams(0.2, 0.2, 0.5, 0.01, 0.5, 3e-4, 0.9, 0.999, 1e-8, 0.0, 1, 2)
    pg_hp = PGHparams(0.01, 0.5, 3e-4, 0.9, 0.999, 1e-8, 1, 0)
    for dims, B, arms in CASES:
        D, A = dims[0], dims[3]
        d = MlpDims(*dims)
        P = int(lib.gs_mlp_param_count(d))
        g = torch.Generator(device="cpu").manual_seed(1234 + B + D)
        T, N = 8, max(2048, B)
        roll = dict(obs=torch.randn(T, N, D, generator=g), actions=torch.randint(0, A, (T, N), generator=g),
                    logprobs=-torch.rand(T, N, generator=g) - 0.2, values=torch.randn(T, N, generator=g),
                    advantages=torch.randn(T, N, generator=g), returns=torch.randn(T, N, generator=g))
        roll = {k: v.to(dev).contiguous() for k, v in roll.items()}
        view = RolloutView(*(roll[k].data_ptr() for k in ("obs", "actions", "logprobs", "values", "advantages", "returns")),
                           T, N)
        idx = torch.randint(0, T * N, (n * B,), generator=g, dtype=torch.int32).to(dev)
        p0 = (0.05 * torch.randn(P, generator=g)).to(dev)
        state = {}
        for arm in arms:
            nbytes = int({"rows": lambda: lib.gs_ppo_rows_workspace_bytes(d, B),
                          "pg": lambda: lib.gs_pg_update_workspace_bytes(d, B),
                          "chain": lambda: lib.gs_ppo_update_workspace_bytes(d, B, n)}[arm]())
            if nbytes == 0:
                raise SystemExit(f"{arm}: {dims} at B = {B} is not served")
            z = lambda: torch.zeros(P, device=dev)  # noqa: E731
            state[arm] = dict(p=p0.clone(), g=z(), m=z(), v=z(), ws=torch.zeros(nbytes, dtype=torch.uint8, device=dev),
                              met=torch.zeros(n, 40, device=dev), stop=torch.zeros(1, dtype=torch.int32, device=dev),
                              step=0)

        def window(arm):
            s = state[arm]
            st = torch.cuda.current_stream().cuda_stream
            head = (s["p"].data_ptr(), s["g"].data_ptr(), s["m"].data_ptr(), s["v"].data_ptr(), d)
            if arm == "rows":
                check(lib.gs_ppo_rows_update(*head, ppo_hp, view, idx.data_ptr(), B, n, s["step"], s["met"].data_ptr(),
                                             s["stop"].data_ptr(), s["ws"].data_ptr(), s["ws"].numel(), None, st), arm)
            elif arm == "pg":
                check(lib.gs_pg_update(*head, pg_hp, view, idx.data_ptr(), B, n, s["step"], s["met"].data_ptr(),
                                       s["ws"].data_ptr(), s["ws"].numel(), None, st), arm)
            else:
                check(lib.gs_ppo_update(*head, ppo_hp, view, idx.data_ptr(), B, n, s["step"], s["met"].data_ptr(),
                                        s["stop"].data_ptr(), s["ws"].data_ptr(), s["ws"].numel(), None, 1, st), arm)
            s["step"] += n

        def timed(arm):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            window(arm)
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1) * 1000.0 / n

        for _ in range(a.warmup):
            for arm in arms:
                window(arm)
        torch.cuda.synchronize()
        us = {arm: [] for arm in arms}
        for _ in range(a.repeats):
            for arm in arms:
                us[arm].append(timed(arm))
        row = {"dims": list(dims), "batch": B}
        for arm in arms:
            if not torch.isfinite(state[arm]["met"]).all() or not torch.isfinite(state[arm]["p"]).all():
                raise SystemExit(f"{arm}: non-finite records or parameters at {dims}, B = {B}")
            med = statistics.median(us[arm])
            row[arm] = {"step_us": [round(x, 3) for x in us[arm]], "median_us": round(med, 3),
                        "spread_us": round(max(us[arm]) - min(us[arm]), 3), "rows_per_s": round(B / med * 1e6)}
        if (dims, B) in GATED:
            row["gate_rows_le_pg_plus_pg_spread"] = bool(row["rows"]["median_us"] <= row["pg"]["median_us"] + row["pg"]["spread_us"])
        out["results"].append(row)
        print(json.dumps(row), flush=True)
        del state, roll
    out["gate"] = all(r.get("gate_rows_le_pg_plus_pg_spread", True) for r in out["results"])
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    print("gate:", out["gate"])


if __name__ == "__main__":
    main()
