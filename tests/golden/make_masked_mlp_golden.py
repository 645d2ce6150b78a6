"""Generate the masked-MLP fixtures FROM THE REFERENCE ITSELF (build container only; see make_golden.py
for the import stubs this reuses).  Writes next to this script:

  masked_mlp.npz            per case (`small`: 12-128-128-18, `tiny`: 12-64-18), the reference's
                            MLPActorCritic(valid_actions=[0, 3, 4]) (utils/models.py:285-346) on a 64-row
                            batch whose actions come from the model's own distribution:
                              state/<key>          the state dict (the reference's init, the policy head
                                                   scaled by 100 so the valid logits differ by O(1) and not
                                                   by the 0.01-gain head's O(0.01))
                              batch/<field>        observations, actions, logprobs, values, advantages, returns
                              act/{actions,logprobs,values}   policy_act(deterministic=True)
                                                   (utils/policy_ops.py:14-34)
                              loss, metric_names / metric_values   PPOAgent.losses_for_batch's outputs
                                                   (agents/ppo/ppo_agent.py:21-152) under HP below
                              new_logprobs, entropy_rows      the distribution's per-row log_prob / entropy
                              grads                the flat parameter gradient after loss.backward()
  config_pong_objects.json  every field the reference's load_config resolves for ALE-Pong-v5's
                            objects_ppo / objects_deterministic_ppo (n_envs is written in the yaml: 32)

Usage: python tests/golden/make_masked_mlp_golden.py [model] [configs]
"""
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as G  # noqa: E402  (reference on sys.path, third-party stubs, torch)
import torch  # noqa: E402

from utils.models import MLPActorCritic  # noqa: E402
from utils.policy_ops import policy_act  # noqa: E402

VALID = [0, 3, 4]
CASES = {"small": (12, (128, 128), 18), "tiny": (12, (64,), 18)}
B = 64
HP = dict(normalize="batch", clip=0.2, clip_vf=0.2, vf_coef=0.5, ent_coef=0.01)       # tests/mlp_cases.HP
CONFIG_IDS = (("ALE-Pong-v5", "objects_ppo"), ("ALE-Pong-v5", "objects_deterministic_ppo"))


def make_model():
    out = {"valid": np.array(VALID, np.int64)}
    for s, (tag, (D, hidden, A)) in enumerate(CASES.items()):
        torch.manual_seed(20270 + s)
        model = MLPActorCritic(input_shape=(D,), hidden_dims=hidden, output_shape=(A,), activation="relu",
                               valid_actions=list(VALID))
        with torch.no_grad():
            model.policy_head.weight.mul_(100.0)
        for k, v in model.state_dict().items():
            out[f"{tag}/state/{k}"] = v.detach().numpy().copy()
        obs = torch.randn(B, D)
        with torch.no_grad():
            dist, value = model(obs)
            actions = dist.sample()
            assert set(actions.tolist()) <= set(VALID) and len(set(actions.tolist())) == len(VALID)
            lp = dist.log_prob(actions)
        # old log-probs / values off the current ones, so ratios straddle the clip range and value deltas
        # the value clip range (tests/mlp_cases.case's recipe)
        batch = types.SimpleNamespace(observations=obs, actions=actions, logprobs=lp + 0.15 * torch.randn(B),
                                      values=value + 0.3 * torch.randn(B), advantages=0.5 + 2.0 * torch.randn(B),
                                      returns=value + torch.randn(B))
        for f in ("observations", "actions", "logprobs", "values", "advantages", "returns"):
            out[f"{tag}/batch/{f}"] = getattr(batch, f).numpy().copy()
        a, alp, av = policy_act(model, obs, deterministic=True)
        out[f"{tag}/act/actions"], out[f"{tag}/act/logprobs"], out[f"{tag}/act/values"] = (
            a.numpy().copy(), alp.numpy().copy(), av.numpy().copy())
        assert set(a.tolist()) <= set(VALID)
        agent, recs = G._agent(model, HP)
        model.zero_grad()
        res = agent.losses_for_batch(batch, 0)
        assert res["early_stop_epoch"] is False
        res["loss"].backward()
        m = {k: float(v) for k, v in recs[0].items()}
        assert 0 < m["opt/ppo/clip_fraction"] < 1 and 0 < m["opt/ppo/clip_fraction_vf"] < 1, m
        out[f"{tag}/loss"] = np.float32(res["loss"].item())
        out[f"{tag}/metric_names"] = np.array(sorted(m))
        out[f"{tag}/metric_values"] = np.array([m[k] for k in sorted(m)], np.float64)
        with torch.no_grad():
            dist, _ = model(obs)
            out[f"{tag}/new_logprobs"] = dist.log_prob(actions).numpy().copy()
            out[f"{tag}/entropy_rows"] = dist.entropy().numpy().copy()
        out[f"{tag}/grads"] = G._flat_grads(model)
        rows = model.policy_head.weight.grad.numpy()
        invalid = [a for a in range(A) if a not in VALID]
        assert not rows[invalid].any() and not model.policy_head.bias.grad.numpy()[invalid].any()
    path = os.path.join(HERE, "masked_mlp.npz")
    np.savez_compressed(path, **out)
    print("masked_mlp.npz written:", len(out), "arrays,", os.path.getsize(path), "bytes")


def make_configs():
    import dataclasses
    rec = {}
    cores, os.cpu_count = os.cpu_count, (lambda: 7)        # n_envs must not come from "auto"
    try:
        for env, var in CONFIG_IDS:
            c = G.load_config(env, var)
            d = {k: getattr(v, "value", v) for k, v in dataclasses.asdict(c).items()}
            d["algo_id"] = c.algo_id
            assert d["n_envs"] == 32
            d.update({k: v for k, v in vars(c).items() if "_schedule" in k and not k.startswith("_")})
            d["_hidden_dims"] = list(c.hidden_dims)
            d["_n_actions"] = c.spec.get("action_space", {}).get("discrete")
            d["_valid_actions"] = c.spec.get("action_space", {}).get("valid")
            rec[f"{env}:{var}"] = json.loads(json.dumps(d, default=lambda o: getattr(o, "value", str(o))))
    finally:
        os.cpu_count = cores
    with open(os.path.join(HERE, "config_pong_objects.json"), "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print("config_pong_objects.json written")


if __name__ == "__main__":
    for name in (sys.argv[1:] or ["model", "configs"]):
        globals()[f"make_{name}"]()
