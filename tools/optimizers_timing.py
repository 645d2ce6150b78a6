"""Per-minibatch times of Adam / AdamW / SGD (include/gsamd.h GS_HP_OPT_*) on one MI355X: gs_ppo_update at
the C2 chain shape (captured graph; GS_LAGGED_ADAM=0 in the environment puts the Adam arm on the same
non-lagged chain as the other two), gs_ppo_rows_update at 4-256-256-2, B = 2048, and gs_cnn_ppo_update
at NatureCNN size.  HIP events around one call of N minibatches; the arms alternate inside every repeat.

  python tools/optimizers_timing.py --json OUT.json        all three
  python tools/optimizers_timing.py --only chain | cnn     one of them, the result on stdout (cnn: the
                                                           run to put under a kernel trace for k_clip_adam_flat)
profiles/optimizers_timing.json holds a run of each and the bench.py A/B of the unchanged Adam path."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "gymnasium-solver_amd")):
    sys.path.insert(0, p)

import numpy as np
import torch

from gsamd._lib import (GS_HP_OPT_ADAMW, GS_HP_OPT_SGD, GS_NUM_METRICS, CnnDims, MlpDims, PPOHparams, RolloutView,
                        RolloutViewU8, check, lib)

dev = torch.device("cuda:0")
ARMS = {"adam": 0, "adamw": GS_HP_OPT_ADAMW, "sgd": GS_HP_OPT_SGD}
REPEATS, WARM = 5, 2


def hp(flags, lr=3e-4):
    return PPOHparams(0.2, 0.2, 0.5, 0.01, 0.5, lr, 0.9, 0.999, 1e-8, 0.0, 1, flags)


def stream():
    return torch.cuda.current_stream().cuda_stream


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3      # us


def measure(calls, steps):
    """calls: arm -> zero-argument call of `steps` minibatches"""
    for _ in range(WARM):
        for fn in calls.values():
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in calls}
    for _ in range(REPEATS):
        for k, fn in calls.items():
            out[k].append(round(timed(fn) / steps, 3))
    return {k: {"step_us": v, "median_us": float(np.median(v)), "min_us": min(v), "max_us": max(v)} for k, v in out.items()}


def mlp_case(dims, T, N):
    rng = np.random.default_rng(1)
    D, H1, H2, A = dims
    md = MlpDims(*dims)
    P = int(lib.gs_mlp_param_count(md))
    t = lambda x, dt=None: torch.as_tensor(np.ascontiguousarray(x)).to(dt or torch.float32).to(dev)  # noqa: E731
    bufs = [t(rng.standard_normal((T, N, D))), t(rng.integers(0, A, (T, N)), torch.int64),
            t(-0.7 + 0.05 * rng.standard_normal((T, N))), t(0.1 * rng.standard_normal((T, N))),
            t(rng.standard_normal((T, N))), t(rng.standard_normal((T, N)))]
    view = RolloutView(*(b.data_ptr() for b in bufs), T, N)
    p0 = t(0.05 * rng.standard_normal(P))
    return md, P, bufs, view, p0


def chain():
    dims, B, T, N = (4, 256, 256, 2), 256, 32, 4096
    steps = T * N // B                  # 512 minibatches: one epoch of the C2 rollout
    md, P, bufs, view, p0 = mlp_case(dims, T, N)
    idx = torch.randperm(T * N, device=dev).to(torch.int32)
    ws = torch.zeros(int(lib.gs_ppo_update_workspace_bytes(md, B, steps)), dtype=torch.uint8, device=dev)
    met = torch.zeros(steps, GS_NUM_METRICS, device=dev)
    stop = torch.zeros(1, dtype=torch.int32, device=dev)
    st = {k: [p0.clone(), torch.zeros(P, device=dev), torch.zeros(P, device=dev), torch.zeros(P, device=dev)] for k in ARMS}

    def call(k):
        p, g, m, v = st[k]
        return lambda: check(lib.gs_ppo_update(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), md, hp(ARMS[k]), view,
                                               idx.data_ptr(), B, steps, 0, met.data_ptr(), stop.data_ptr(), ws.data_ptr(),
                                               ws.numel(), None, 1, stream()), "gs_ppo_update")
    r = measure({k: call(k) for k in ARMS}, steps)
    return {"what": "gs_ppo_update, captured graph, 4-256-256-2, B = 256, %d minibatches per call; Adam runs the lagged "
                    "chain, AdamW / SGD the fused chain with a k_clip_adam launch per minibatch" % steps, **r}


def rows():
    dims, B, T, N = (4, 256, 256, 2), 2048, 32, 1024
    steps = T * N // B                  # 16
    md, P, bufs, view, p0 = mlp_case(dims, T, N)
    idx = torch.randperm(T * N, device=dev).to(torch.int32)
    ws = torch.zeros(int(lib.gs_ppo_rows_workspace_bytes(md, B)), dtype=torch.uint8, device=dev)
    met = torch.zeros(steps, GS_NUM_METRICS, device=dev)
    stop = torch.zeros(1, dtype=torch.int32, device=dev)
    st = {k: [p0.clone(), torch.zeros(P, device=dev), torch.zeros(P, device=dev), torch.zeros(P, device=dev)] for k in ARMS}

    def call(k):
        p, g, m, v = st[k]
        return lambda: check(lib.gs_ppo_rows_update(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), md, hp(ARMS[k]),
                                                    view, idx.data_ptr(), B, steps, 0, met.data_ptr(), stop.data_ptr(),
                                                    ws.data_ptr(), ws.numel(), None, stream()), "gs_ppo_rows_update")
    r = measure({k: call(k) for k in ARMS}, steps)
    return {"what": "gs_ppo_rows_update, 4-256-256-2, B = 2048, %d minibatches per call (three launches each)" % steps, **r}


def cnn():
    B, T, N, steps = 256, 8, 128, 4
    rng = np.random.default_rng(2)
    cd = CnnDims(4, 84, 84, 18, 512, 0)
    P = int(lib.gs_cnn_param_count(cd))
    t = lambda x, dt: torch.as_tensor(np.ascontiguousarray(x)).to(dt).to(dev)  # noqa: E731
    bufs = [t(rng.integers(0, 256, (T, N, 4, 84, 84)), torch.uint8), t(rng.integers(0, 18, (T, N)), torch.int64),
            t(-2.9 + 0.05 * rng.standard_normal((T, N)), torch.float32), t(0.1 * rng.standard_normal((T, N)), torch.float32),
            t(rng.standard_normal((T, N)), torch.float32), t(rng.standard_normal((T, N)), torch.float32)]
    view = RolloutViewU8(*(b.data_ptr() for b in bufs), T, N)
    p0 = t(0.01 * rng.standard_normal(P), torch.float32)
    idx = torch.randperm(T * N, device=dev).to(torch.int32)
    ws = torch.zeros(int(lib.gs_cnn_workspace_bytes(cd, B)), dtype=torch.uint8, device=dev)
    met = torch.zeros(steps, GS_NUM_METRICS, device=dev)
    stop = torch.zeros(1, dtype=torch.int32, device=dev)
    st = {k: [p0.clone(), torch.zeros(P, device=dev), torch.zeros(P, device=dev), torch.zeros(P, device=dev)] for k in ARMS}

    def call(k):
        p, g, m, v = st[k]
        return lambda: check(lib.gs_cnn_ppo_update(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), cd, hp(ARMS[k]),
                                                   view, idx.data_ptr(), B, steps, 0, met.data_ptr(), stop.data_ptr(),
                                                   ws.data_ptr(), None, stream()), "gs_cnn_ppo_update")
    r = measure({k: call(k) for k in ARMS}, steps)
    return {"what": "gs_cnn_ppo_update, NatureCNN 4x84x84 -> 18 actions (%d parameters), B = %d, %d minibatches per call: "
                    "the whole step (k_clip_adam_flat is its last launch)" % (P, B, steps), **r}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None, help="write the result here as well as to stdout")
    ap.add_argument("--only", choices=("chain", "cnn"), default=None)
    args = ap.parse_args()
    if args.only:
        out = chain() if args.only == "chain" else cnn()
    else:
        out = {"unit": "us per minibatch (one call of N minibatches / N), HIP events; arms alternate inside each repeat",
               "repeats": REPEATS, "warmup_calls": WARM, "device": torch.cuda.get_device_name(0),
               "chain_c2": chain(), "rows": rows(), "nature_cnn_step": cnn()}
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps(out))
